"""The keyframe map sharded across ranks BEHIND Pipeline.compute (Pipeline::setShard, sharded.shard_pipeline; DESIGN.md
section 7) — 8, 4 and 2 ranks on the ONE GPU of the test box, each a fresh process with its own Pipeline on its own slice of
the CU mask (MADICP_CU_MASK=i/n), every rank fed the same full-size scans in the same order, over the host-staged transport
and over the peer mailboxes.  NOTHING here crossed xGMI: functional coverage, not a scaling measurement.

Drive A (deskew = false, 44 frames of scene 9 at 1 m per frame, p_th 0.95, 4 keyframes — parameters of
tests/test_gpu_frontend_oracle.py, the frame count raised until the ORACLE alone promotes at least num_keyframes + 3 times;
with 4 keyframes over eight ranks at least four ranks own no tree at every frame):
  * every rank's currentPose() is bit-equal to every other rank's at every frame; keyframeID / isMapUpdated / currentID equal;
  * those sequences are the oracle pipeline's, and every pose is within 1e-5 m / 1e-5 rad of the oracle's;
  * numLocalKeyframes() on rank r is what keyframe_owner deals it from the global window, the counts sum to numKeyframes();
  * modelLeaves() on the last frame: the same shape on every rank, and the deviation from the UNSHARDED product Pipeline (run
    in the parent on the same scans) is printed, with the worst pose deviation from it — measured, not asserted beyond the
    oracle bar.
Drive B (deskew = true, 20 frames, 4 ranks, host transport): ranks bit-equal to each other, ids equal — no oracle bar: the
reference does not reproduce itself there (tests/envelope.py).
Legality: setShard after the first compute raises; an unsharded Pipeline created after sharded.unshard in the same process
gives the poses of one that never saw a communicator, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import envelope as E
import oracle_lib as O
from fixtures import B_MAX, B_MIN, B_RATIO, RHO_KER, full_scan
from mad_icp_amd import sharded

pytestmark = pytest.mark.gpu

SCENE, STEP, P_TH, KF = 9, 1.0, 0.95, 4
N_FRAMES_A, N_FRAMES_B, N_AFTER = 44, 20, 5
ARGS_A = (10.0, False, B_MAX, RHO_KER, P_TH, B_MIN, B_RATIO, KF, 16, False)
ARGS_B = (10.0, True, B_MAX, RHO_KER, P_TH, B_MIN, B_RATIO, KF, 16, False)


def _window(n_promoted, kf=KF):
    """the ordinals in the global window after `n_promoted` keyframes (the first scan included)"""
    return range(max(0, n_promoted - kf), n_promoted)


@pytest.fixture(scope="module")
def drive(natives, tmp_path_factory):
    """The scans once, on disk for the workers; the oracle pipeline and the UNSHARDED product Pipeline over them."""
    from mad_icp.src.pybind import pypeline

    scans = [full_scan(SCENE, STEP * i, 4000 + 97 * SCENE + i) for i in range(N_FRAMES_A)]
    path = str(tmp_path_factory.mktemp("shard_pipeline") / "scans.npz")
    np.savez(path, **{"s%d" % i: s for i, s in enumerate(scans)})
    op = O.Pipeline(*ARGS_A)
    orc = dict(pose=[], kf=[], upd=[], cur=[])
    for i, s in enumerate(scans):
        op.compute(0.1 * i, s)
        orc["pose"].append(np.asarray(op.currentPose()).copy())
        orc["kf"].append(int(op.keyframeID()))
        orc["upd"].append(bool(op.isMapUpdated()))
        orc["cur"].append(int(op.currentID()))
    # the drive exercises what it is here for, by the ORACLE's own decisions: promotions past the window's size (evictions),
    # and — eight ranks — a rank that owns no tree at some frame
    promotions = int(np.sum(orc["upd"][1:]))
    assert promotions >= KF + 3, promotions
    assert promotions + 1 - KF >= 3  # evictions
    n_prom = np.cumsum(orc["upd"])
    assert any(sum(1 for o in _window(int(p)) if sharded.keyframe_owner(o, 8) == r) == 0 for p in n_prom for r in range(8))
    gp = pypeline.Pipeline(*ARGS_A)
    uns = dict(pose=[])
    for i, s in enumerate(scans):
        gp.compute(0.1 * i, s)
        uns["pose"].append(np.asarray(gp.currentPose()).copy())
    uns["model"] = np.asarray(gp.modelLeaves()).copy()
    del gp
    return dict(path=path, oracle=orc, unsharded=uns)


def _drive_pipeline(pipe, z, n_frames):
    rec = dict(pose=[], kf=[], upd=[], cur=[], n_local=[], n_kf=[])
    for i in range(n_frames):
        pipe.compute(0.1 * i, z["s%d" % i])
        rec["pose"].append(np.asarray(pipe.currentPose()).copy())
        rec["kf"].append(int(pipe.keyframeID()))
        rec["upd"].append(bool(pipe.isMapUpdated()))
        rec["cur"].append(int(pipe.currentID()))
        rec["n_local"].append(int(pipe.numLocalKeyframes()))
        rec["n_kf"].append(int(pipe.numKeyframes()))
    return {k: np.array(v) for k, v in rec.items()}


def _worker(rank, world, port, path, out, plan):
    """plan: [(tag, pipeline args, transport, frames)] — one sharded Pipeline each, one after the other, in this process"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["MADICP_CU_MASK"] = "%d/%d" % (rank, world)
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mad_icp.src.pybind import pypeline

        z = np.load(path)
        res = {}
        # a Pipeline that never saw a communicator, in this process and on this slice of the CU mask
        before = pypeline.Pipeline(*ARGS_A)
        res["before_pose"] = _drive_pipeline(before, z, N_AFTER)["pose"]
        try:
            before.setShard(rank, world)
            res["late_setshard"] = "no error"
        except RuntimeError as e:
            res["late_setshard"] = "RuntimeError: %s" % e
        del before
        for tag, args, transport, n_frames in plan:
            pipe = pypeline.Pipeline(*args)
            pctx = sharded.shard_pipeline(pipe, transport=transport, allow_coarse=True)
            assert (pipe.shardRank(), pipe.shardWorld()) == (rank, world)
            pctx.set_option("comm_timeout_ms", 60000)
            for k, v in _drive_pipeline(pipe, z, n_frames).items():
                res["%s_%s" % (tag, k)] = v
            res[tag + "_model"] = np.asarray(pipe.modelLeaves()).copy()
            res[tag + "_current"] = np.asarray(pipe.currentLeaves()).copy()
            del pipe
            sharded.unshard(pctx)
            assert pctx.get_option("comm_ranks") == 0 and pctx.get_option("shard_p2p") == 0
        after = pypeline.Pipeline(*ARGS_A)
        assert after.shardWorld() == 1
        res["after_pose"] = _drive_pipeline(after, z, N_AFTER)["pose"]
        del after
        np.savez(out % rank, **res)
    finally:
        dist.destroy_process_group()


def _spawn(world, path, tmp_path, plan, salt):
    out = str(tmp_path / "rank%d.npz")
    port = 29500 + ((os.getpid() * 11 + world * 17 + salt) % 3000)
    mp.spawn(_worker, args=(world, port, path, out, plan), nprocs=world, join=True)  # (a failing worker raises here: no retry)
    return [np.load(out % r) for r in range(world)]


def _legality(R, drive):
    for r in R:
        assert str(r["late_setshard"]).startswith("RuntimeError") and "first compute" in str(r["late_setshard"]), str(r["late_setshard"])
        # unsharded again after unshard: the Pipeline that never saw a communicator, bit for bit — in this process, and in the
        # parent's (whose poses are the unsharded product's over the whole drive)
        assert np.array_equal(r["after_pose"], r["before_pose"])
        assert np.array_equal(r["after_pose"], np.array(drive["unsharded"]["pose"][:N_AFTER]))


@pytest.mark.parametrize("world", [8, 4, 2])
def test_drive_a_sharded_pipeline_over_world_ranks_one_gpu(drive, tmp_path, world, capsys):
    orc, uns = drive["oracle"], drive["unsharded"]
    plan = [("host", ARGS_A, "host", N_FRAMES_A), ("p2p", ARGS_A, "p2p", N_FRAMES_A)]
    R = _spawn(world, drive["path"], tmp_path, plan, 1)
    _legality(R, drive)
    report = []
    for t in ("host", "p2p"):
        # across ranks: poses bit-equal at every frame, decisions identical
        for r in R[1:]:
            assert np.array_equal(R[0][t + "_pose"], r[t + "_pose"]), t
            for key in ("kf", "upd", "cur", "n_kf"):
                assert np.array_equal(R[0][t + "_" + key], r[t + "_" + key]), (t, key)
        r0 = R[0]
        # against the oracle: the same decisions, every pose within the project's bar for this path
        assert list(r0[t + "_kf"]) == orc["kf"] and list(r0[t + "_upd"]) == orc["upd"] and list(r0[t + "_cur"]) == orc["cur"], t
        worst_t = worst_a = 0.0
        for i in range(N_FRAMES_A):
            dt, da = E.pose_dev(orc["pose"][i], r0[t + "_pose"][i])
            worst_t, worst_a = max(worst_t, dt), max(worst_a, da)
        print("[%s, world %d] worst deviation from the oracle pipeline over %d frames: %.3e m / %.3e rad" % (t, world, N_FRAMES_A, worst_t, worst_a))
        assert worst_t <= 1e-5 and worst_a <= 1e-5, (t, worst_t, worst_a)
        # ownership: what keyframe_owner deals each rank from the global window, frame by frame
        n_prom = np.cumsum(r0[t + "_upd"])
        some_rank_empty = False
        for i in range(N_FRAMES_A):
            win = _window(int(n_prom[i]))
            assert int(r0[t + "_n_kf"][i]) == len(win), (t, i)
            counts = [int(r[t + "_n_local"][i]) for r in R]
            assert counts == [sum(1 for o in win if sharded.keyframe_owner(o, world) == q) for q in range(world)], (t, i, counts)
            assert sum(counts) == int(r0[t + "_n_kf"][i])
            some_rank_empty |= min(counts) == 0
        if world == 8:
            assert some_rank_empty
        # the full map on every rank
        for r in R[1:]:
            assert r[t + "_model"].shape == r0[t + "_model"].shape and r[t + "_current"].shape == r0[t + "_current"].shape, t
        assert r0[t + "_model"].shape == uns["model"].shape, (t, r0[t + "_model"].shape, uns["model"].shape)
        assert r0[t + "_model"].shape[0] > 0 and r0[t + "_current"].shape[0] > 0
        between = max(float(np.abs(r[t + "_model"] - r0[t + "_model"]).max()) for r in R[1:])
        d_model = float(np.abs(r0[t + "_model"] - uns["model"]).max())
        du_t = du_a = 0.0
        for i in range(N_FRAMES_A):
            dt, da = E.pose_dev(uns["pose"][i], r0[t + "_pose"][i])
            du_t, du_a = max(du_t, dt), max(du_a, da)
        report.append("[sharded Pipeline, %s transport, world %d, %d frames x %d points, %d keyframes] vs oracle %.2e m / %.2e rad; vs the "
                      "unsharded product: poses %.2e m / %.2e rad, modelLeaves() (%d leaves) %.2e m; modelLeaves() between ranks %.2e m; "
                      "trees per rank on the last frame %s"
                      % (t, world, N_FRAMES_A, drive_points(drive), KF, worst_t, worst_a, du_t, du_a, uns["model"].shape[0], d_model,
                         between, [int(r[t + "_n_local"][-1]) for r in R]))
    with capsys.disabled():
        print()
        for line in report:
            print(line)


def drive_points(drive):
    return int(np.load(drive["path"])["s0"].shape[0])


def test_drive_b_deskewed_ranks_agree(drive, tmp_path, capsys):
    world = 4
    R = _spawn(world, drive["path"], tmp_path, [("deskew", ARGS_B, "host", N_FRAMES_B)], 2)
    _legality(R, drive)
    for r in R[1:]:
        assert np.array_equal(R[0]["deskew_pose"], r["deskew_pose"])
        for key in ("kf", "upd", "cur", "n_kf"):
            assert np.array_equal(R[0]["deskew_" + key], r["deskew_" + key]), key
        assert r["deskew_model"].shape == R[0]["deskew_model"].shape
    n_prom = np.cumsum(R[0]["deskew_upd"])
    for i in range(N_FRAMES_B):
        win = _window(int(n_prom[i]))
        counts = [int(r["deskew_n_local"][i]) for r in R]
        assert counts == [sum(1 for o in win if sharded.keyframe_owner(o, world) == q) for q in range(world)], (i, counts)
    assert np.linalg.norm(R[0]["deskew_pose"][-1][:3, 3]) > 5.0  # (the drive moved)
    with capsys.disabled():
        print("\n[sharded Pipeline, deskew = true, host transport, world 4, %d frames] ranks bit-equal; %d promotions"
              % (N_FRAMES_B, int(n_prom[-1]) - 1))


def test_set_shard_after_the_first_compute_raises(drive):
    from mad_icp.src.pybind import pypeline

    z = np.load(drive["path"])
    p = pypeline.Pipeline(*ARGS_A)
    p.setShard(0, 1)
    p.compute(0.0, z["s0"])
    with pytest.raises(RuntimeError, match="first compute"):
        p.setShard(0, 1)
    with pytest.raises(RuntimeError, match="first compute"):
        p.setShard(0, 2)
    assert p.shardWorld() == 1 and p.numLocalKeyframes() == 1 and p.numKeyframes() == 1


def test_sharded_compute_without_a_communicator_is_refused(drive):
    """setShard(r, w) without the communicator in the process-wide context would register against a part of the map alone:
    the first registration refuses instead."""
    from mad_icp.src.pybind import pypeline

    z = np.load(drive["path"])
    p = pypeline.Pipeline(*ARGS_A)
    p.setShard(0, 2)
    p.compute(0.0, z["s0"])  # (the first scan only initialises)
    with pytest.raises(RuntimeError, match="communicator"):
        p.compute(0.1, z["s1"])
