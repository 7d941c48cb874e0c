"""The host side of the sharded keyframe map behind Pipeline.compute, without a device:

  * the ownership rule restated in C++ (csrc/common/keyframe_owner.h, exported as madicp_host_keyframe_owner) IS
    sharded.keyframe_owner, and deals evenly: every window of 2 * world consecutive ordinals gives each rank exactly two;
  * the Pipeline.setShard surface (construction needs no device: tests/test_boundary.py builds Pipelines the same way);
  * capi.Context.borrowed / madicp_host_device_ctx: the way to the process-wide context exists (on a box without a GPU the
    call fails loudly, like every device entry point);
  * the window bookkeeping Pipeline pushes and evicts its keyframes by (csrc/host/keyframe_ledger.h), driven through the host
    C ABI's test hook over scripted promotion sequences, one ledger per rank: after every promotion the ranks' local sets are
    disjoint and their union is exactly the last num_keyframes ordinals.

The GPU half is tests/test_gpu_shard_pipeline.py."""
import ctypes
import os

import numpy as np
import pytest

from fixtures import B_MAX, B_MIN, B_RATIO, RHO_KER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pypeline(natives):
    from mad_icp.src.pybind import pypeline as m

    return m


def test_cxx_owner_is_the_python_owner(natives):
    from mad_icp_amd import capi, sharded

    for w in range(1, 17):
        got = [capi.host_keyframe_owner(k, w) for k in range(4096)]
        want = [sharded.keyframe_owner(k, w) for k in range(4096)]
        assert got == want, w
        assert min(got) == 0 and max(got) == w - 1


def test_every_window_of_two_rows_gives_each_rank_two(natives):
    """num_keyframes = 16 over eight ranks: two trees per rank at every frame — and the same for every world size."""
    from mad_icp_amd import capi

    for w in range(1, 17):
        owner = np.array([capi.host_keyframe_owner(k, w) for k in range(4096)])
        for start in range(4096 - 2 * w + 1):
            counts = np.bincount(owner[start:start + 2 * w], minlength=w)
            assert (counts == 2).all(), (w, start, counts)


def test_owner_bad_arguments(natives):
    from mad_icp_amd import capi

    for k, w in ((-1, 8), (0, 0), (5, -3), (-7, -1), (-(2 ** 40), 4)):
        assert capi.host_keyframe_owner(k, w) == -1, (k, w)
    assert capi.host_keyframe_owner(2 ** 40, 8) in range(8)  # (a 64-bit ordinal is fine)


def _pipeline(pypeline, realtime=False, num_keyframes=4):
    return pypeline.Pipeline(10.0, False, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, num_keyframes, 4, realtime)


def test_set_shard_surface(pypeline):
    for name in ("setShard", "shardRank", "shardWorld", "numLocalKeyframes"):
        assert hasattr(pypeline.Pipeline, name), name
    p = _pipeline(pypeline)
    assert p.shardWorld() == 1 and p.shardRank() == 0 and p.numLocalKeyframes() == 0
    p.setShard(0, 1)  # (exactly the unsharded Pipeline)
    assert p.shardWorld() == 1
    p.setShard(rank=5, world=8)
    assert (p.shardRank(), p.shardWorld()) == (5, 8)
    for rank, world in ((8, 8), (9, 8), (2, 2), (-1, 8), (0, 0), (0, -2), (-3, -1)):
        with pytest.raises(ValueError):
            p.setShard(rank, world)
    assert (p.shardRank(), p.shardWorld()) == (5, 8)  # (a refused call changes nothing)
    rt = _pipeline(pypeline, realtime=True)
    rt.setShard(0, 1)
    with pytest.raises(ValueError, match="realtime"):
        rt.setShard(0, 2)
    assert rt.shardWorld() == 1
    # the reference's surface is still all there (pypeline.cpp:57-74)
    for name in ("currentPose", "trajectory", "keyframePose", "isInitialized", "isMapUpdated", "currentID", "keyframeID",
                 "modelLeaves", "currentLeaves", "compute"):
        assert hasattr(pypeline.Pipeline, name), name


def test_borrowed_context_and_its_symbol(natives):
    import torch

    from mad_icp_amd import capi

    L = ctypes.CDLL(os.path.join(ROOT, "mad_icp_amd", "libmadicp_host.so"))
    for sym in ("madicp_host_device_ctx", "madicp_host_keyframe_owner"):
        assert hasattr(L, sym), sym
    assert callable(getattr(capi.Context, "borrowed", None))
    assert hasattr(capi.host_lib(), "madicp_host_device_ctx")
    if torch.cuda.is_available():
        return  # (with a device: tests/test_gpu_shard_pipeline.py uses it for real)
    with pytest.raises(capi.MadIcpError):  # no device: loudly, and nothing to destroy afterwards
        capi.Context.borrowed()


def test_shard_pipeline_is_there(natives):
    from mad_icp_amd import sharded

    assert callable(getattr(sharded, "shard_pipeline", None)) and callable(getattr(sharded, "unshard", None))


@pytest.mark.parametrize("num_keyframes", [4, 16])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_ledger_over_scripted_promotions(natives, num_keyframes, world):
    """One ledger per rank, the same 64 promotions on each (every rank of a sharded Pipeline takes the same decisions).

    Balance: a window of K consecutive ordinals is some FULL rows of `world` — each gives every rank exactly one — between a
    partial row at its old end and a partial row at its new end, each of which gives a rank one or nothing.  So a rank holds
    between F and F + 2 trees, F the number of full rows: the counts differ by at most 2, one per partial row (K = 4 over
    three ranks really shows [2, 2, 0]: ordinals 4 5 | 6 7 are the end of a reversed row and the start of a forward one, both
    on ranks 1 and 0).  When K is a multiple of 2 * world the two partial rows run the same way and complement each other:
    every rank holds exactly K / world."""
    from mad_icp_amd import capi, sharded

    n_promotions = 64
    ledgers = [capi.KeyframeLedger(r, world, num_keyframes) for r in range(world)]
    for step in range(n_promotions):
        got = [l.promote() for l in ledgers]
        want_evicted = step - num_keyframes if step >= num_keyframes else None
        owners = 0
        for r, (ordinal, local, evicted) in enumerate(got):
            assert ordinal == step and evicted == want_evicted, (step, r, ordinal, evicted)
            assert local == (sharded.keyframe_owner(step, world) == r)
            owners += int(local)
        assert owners == 1
        last = list(range(max(0, step + 1 - num_keyframes), step + 1))
        local_sets, counts = [], []
        for r, l in enumerate(ledgers):
            ordinals, local = l.window()
            assert list(ordinals) == last, (step, r)  # the GLOBAL window: the same on every rank
            mine = set(int(o) for o in ordinals[local])
            assert mine == set(o for o in last if sharded.keyframe_owner(o, world) == r)
            assert l.num_local() == len(mine)
            local_sets.append(mine)
            counts.append(len(mine))
        union = set().union(*local_sets)
        assert union == set(last) and sum(counts) == len(last), (step, counts)  # exactly the window, and disjoint
        assert max(counts) - min(counts) <= 2, (step, counts)
        if num_keyframes % (2 * world) == 0 and len(last) == num_keyframes:
            assert counts == [num_keyframes // world] * world, (step, counts)


def test_ledger_bad_arguments(natives):
    from mad_icp_amd import capi

    for rank, world, kf in ((2, 2, 4), (-1, 2, 4), (0, 0, 4), (0, 2, 0)):
        with pytest.raises(ValueError):
            capi.KeyframeLedger(rank, world, kf)
    L = capi.host_lib()
    assert L.madicp_host_debug_ledger_promote(None, None, None) == -1
    assert L.madicp_host_debug_ledger_window(None, None, None, 0) == -1
    assert L.madicp_host_debug_ledger_num_local(None) == -1
