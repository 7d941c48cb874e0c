"""Context.map_score_poses (madicp_map_score_poses: fe::map_score_poses<0 / 1>, and fe::map_slot_rows on maps without the
slot-to-row column) against the restatement (tests/map_score_ref.py: K restated queries of the subsampled cloud), the host twin and
K separate device scoring queries, on plain, attribute, evidence and moments maps: cloud sizes around a wavefront and a workgroup,
pose counts around the kernel's chunk of 64, strides up to n + 1, both reaches, 4 096 points in one voxel, maps after growths, a
prune, a clearing and a wipe, a table whose probes wrap, that the map is only read, and every refusal.  Exact equality everywhere."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_query_ref as Q
import map_score_ref as S
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps and twin are fixtures)
from test_host_map_query import INVALID, KINDS, SPECS, twin  # noqa: F401

pytestmark = pytest.mark.gpu


def everything(m):
    """every column the map has, as bytes"""
    return [c.tobytes() for c in (m.rows(), m.keys(), m.words(), m.evidence(), m.moments()) if c is not None]


@pytest.fixture
def made(ctx, maps, twin):
    """a device map of one of the four kinds and its host twin"""
    return (lambda kind="plain", **k: maps.dev(ctx, **{"voxel": Q.VOXEL, **SPECS[kind], **k})), twin


def test_the_chunk_the_tests_stand_around_is_the_kernels():
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mad_icp_amd", "csrc", "hip", "frontend.hip.h")).read()
    assert int(re.search(r"constexpr int kScoreChunk = (\d+);", src).group(1)) == S.CHUNK == 64
    assert {S.CHUNK - 1, S.CHUNK, S.CHUNK + 1, 2 * S.CHUNK + 2} <= set(S.POSE_COUNTS)


# (a resident cloud always holds a point, so n = 0 is the host twin's case: tests/test_host_map_score.py)
@pytest.mark.parametrize("n", [n for n in S.CLOUD_SIZES if n])
def test_device_score_is_the_restatement_and_the_twin(made, n):
    dev, twin = made
    cloud = Q.sized_cloud(n)
    for kind in KINDS:  # (plain and attr: the transient slot-to-row array)
        d, h = dev(kind), twin(kind)
        Q.build(d, Q.dense_map())
        Q.build(h, Q.dense_map())
        assert d.rows().tobytes() == h.rows().tobytes() and d.keys().tobytes() == h.keys().tobytes()
        for K, stride, reach, md in S.combos(n):
            poses = S.pose_set(K)
            got = S.hold(d, cloud, poses, reach, md, stride, (n, kind, K, stride, reach, md, "device"))
            assert np.array_equal(S.call(h, cloud, poses, reach, md, stride), got), (n, kind, K, stride, reach, md, "twin")


def test_device_score_is_k_separate_scoring_queries(made):
    dev, _ = made
    cloud = Q.sized_cloud(1025)
    for kind in ("plain", "mom"):
        d = dev(kind)
        Q.build(d, Q.dense_map())
        poses = S.pose_set(65)
        for reach, stride in ((0, 1), (1, 1), (1, 7)):
            got = S.call(d, cloud, poses, reach, 0.3, stride)
            sub = np.ascontiguousarray(cloud[::stride])
            with d.resident(sub) as cid:
                want = [d.map.query(cid, X[:9].reshape(3, 3), X[9:], reach, 0.3, False) for X in poses]
            assert np.array_equal(got, np.array(want, np.uint64)), (kind, reach, stride)
            assert got[0, 1] > 50 and got[2, 0] == 0 and np.array_equal(got[0], got[-1])


def test_device_score_of_4096_points_in_one_voxel(made):
    """every lane of every wavefront adds to the same three counters of each pose"""
    dev, _ = made
    steps, asks = Q.one_voxel()
    pts = asks[0][0]
    poses = S.rows_of([E.IDENTITY, (np.eye(3), np.array([Q.VOXEL, 0.0, 0.0])), (np.eye(3), np.array([0.0, 0.0, 2 * Q.VOXEL]))])
    for kind in ("plain", "mom"):
        d = dev(kind)
        Q.build(d, steps)
        for reach in (0, 1):
            got = S.hold(d, pts, poses, reach, 0.3, 1, (kind, reach))
            assert got[0].tolist()[:2] == [4096, 4096] and got[1].tolist()[:2] == [4096, 4096 * reach] and got[2].tolist()[:2] == [4096, 0]


@pytest.mark.parametrize("name", ["faces", "moved", "wiped", "wrapping"])
def test_device_score_on_the_shared_scenarios(made, name):
    dev, twin = made
    steps, asks = Q.named(name)
    cap = dict(max_rows=64) if name == "wrapping" else {}
    for kind in KINDS:
        d, h = dev(kind, **cap), twin(kind, **cap)
        Q.build(d, steps)
        Q.build(h, steps)
        for k, (cloud, R, t) in enumerate(asks):
            poses = S.faces_poses() if name == "faces" else np.concatenate([S.rows_of([(R, t)]), S.pose_set(9, k)])
            for reach in (0, 1):
                for stride in (1, 3):
                    got = S.hold(d, cloud, poses, reach, 0.3, stride, (name, kind, k, reach, stride))
                    assert np.array_equal(S.call(h, cloud, poses, reach, 0.3, stride), got)
                    if name == "wiped":
                        assert not got[:, 1:].any()


def test_device_score_only_reads(made):
    dev, _ = made
    steps, asks = Q.moved()
    more = E.gaussian(500, 99, scale=2.5)
    for kind in KINDS:
        a, b = dev(kind), dev(kind)
        Q.build(a, steps)
        Q.build(b, steps)
        before = everything(a)
        for cloud, R, t in asks:
            for reach in (0, 1):
                S.call(a, cloud, np.concatenate([S.rows_of([(R, t)]), S.pose_set(70)]), reach, 0.3, 2)
        assert everything(a) == before == everything(b)
        assert a.insert(more, *E.IDENTITY, None) == b.insert(more, *E.IDENTITY, None)
        assert everything(a) == everything(b)
        assert a.clear_rays(asks[1][0], *E.IDENTITY, np.array([0.1, -0.2, 0.3])) == b.clear_rays(asks[1][0], *E.IDENTITY, np.array([0.1, -0.2, 0.3]))
        assert everything(a) == everything(b)


def _raw(ctx, mid, cid, poses, K, reach, max_dist, stride, counts, handle=True):
    p = lambda a, ct: None if a is None else a.ctypes.data_as(ct)
    return capi.hip_lib().madicp_map_score_poses(ctx._h if handle else None, mid, cid, p(poses, C.POINTER(C.c_double)), K, reach, max_dist, stride,
                                                 p(counts, C.POINTER(C.c_uint64)))


def test_device_score_refusals_write_nothing(ctx, made):
    dev, _ = made
    plain, mom = dev("plain"), dev("mom")
    pts = np.ascontiguousarray(E.gaussian(40, 1))
    for m in (plain, mom):
        m.insert(pts, *E.IDENTITY, None)
    cid = plain.cloud(pts)
    K = 66
    poses = S.pose_set(K)

    def refused(mid=plain.mid, cloud=cid, poses_=poses, K_=K, reach=1, max_dist=1.0, stride=1, with_counts=True, handle=True):
        counts = np.full(3 * K + 3, S.SENTINEL, np.uint64)
        before = everything(plain) + everything(mom)
        assert _raw(ctx, mid, cloud, poses_, K_, reach, max_dist, stride, counts if with_counts else None, handle) == INVALID
        assert np.all(counts == S.SENTINEL) and everything(plain) + everything(mom) == before

    try:
        refused(handle=False)
        refused(poses_=None)
        refused(with_counts=False)
        refused(mid=987654)
        refused(cloud=987654)
        for K_ in (0, -1, 4097):
            refused(poses_=np.tile(poses[0], (4097, 1)), K_=K_)
        for bad in (np.nan, np.inf, -np.inf):
            for at in (0, 12 * (K - 1) + 11, 12 * (K - 1) + 4):  # (the first entry; t and R of pose K - 1 only)
                P = poses.copy()
                P.reshape(-1)[at] = bad
                for mid in (plain.mid, mom.mid):
                    refused(mid=mid, poses_=P)
        for reach in (-1, 2, 27):
            refused(reach=reach)
        for max_dist in (np.nan, -1.0, -np.inf):
            refused(max_dist=max_dist)
        for stride in (0, -1, -(1 << 62)):
            refused(stride=stride)
        counts = np.full(3 * K + 3, S.SENTINEL, np.uint64)
        assert _raw(ctx, mom.mid, cid, poses, K, 1, np.inf, 1 << 62, counts) == 0  # a stride beyond the cloud: its first point alone
        assert counts[0] == 1 and np.all(counts[3 * K:] == S.SENTINEL)  # (and nothing behind the K rows)
        big = np.tile(poses[:64], (64, 1))
        counts = np.full(3 * 4096 + 3, S.SENTINEL, np.uint64)
        assert _raw(ctx, plain.mid, cid, big, 4096, 0, 0.3, 1, counts) == 0  # the most poses a call takes
        assert np.array_equal(counts[:3 * 4096].reshape(64, 64, 3), np.tile(counts[:3 * 64].reshape(1, 64, 3), (64, 1, 1)))
        assert np.all(counts[3 * 4096:] == S.SENTINEL)
    finally:
        ctx.cloud_release(cid)
