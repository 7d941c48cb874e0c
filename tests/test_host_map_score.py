"""The host twin's pose scoring (madicp_host_map_score, csrc/host/voxel_map.h: VoxelMap::score) against the restatement
(tests/map_score_ref.py: K separate restated queries of the subsampled cloud) on plain, attribute, evidence and moments maps —
exact equality everywhere.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_query_ref as Q
import map_score_ref as S
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)
from test_host_map_query import KINDS, SPECS

INVALID = -1


@pytest.fixture
def twin(maps):
    return lambda kind="plain", **k: maps.host(**{"voxel": Q.VOXEL, "insert_attr": True, **SPECS[kind], **k})


@pytest.mark.parametrize("n", S.CLOUD_SIZES)
def test_host_score_is_the_restatement(twin, n):
    cloud = Q.sized_cloud(n)
    first = None
    for kind in KINDS:
        m = twin(kind)
        Q.build(m, Q.dense_map())
        got = [S.hold(m, cloud, S.pose_set(K), reach, md, stride, (n, kind, K, stride, reach, md)) for K, stride, reach, md in S.combos(n)]
        for K, g in zip((c[0] for c in S.combos(n)), got):
            if K >= 5:
                assert np.array_equal(g[0], g[-1]), (n, kind, K, "the same pose twice")
            if K >= 3:
                assert g[2, 0] == 0, (n, kind, K, "outside the key range: no candidate")
        first = first or got
        assert all(np.array_equal(a, b) for a, b in zip(first, got)), (n, kind)  # the same counts on all four kinds


def test_host_score_counts_something():
    """the scenario is not vacuous: at the cloud's own pose most points match, at the identity fewer"""
    h = capi.HostMap.create(Q.VOXEL, 64, 1 << 20)
    try:
        h.insert(Q.dense_map()[0][1], *E.IDENTITY)
        c = h.score(Q.sized_cloud(1025), S.pose_set(65), 1, 0.3, 1)
        assert c[0, 0] == 1025 and c[0, 1] > 500 and 0 < c[0, 2] < c[0, 1] and c[1, 1] < c[0, 1]
    finally:
        h.close()


@pytest.mark.parametrize("name", ["faces", "moved", "wiped", "wrapping"])
def test_host_score_on_the_shared_scenarios(twin, name):
    steps, asks = Q.named(name)
    for kind in KINDS:
        m = twin(kind, max_rows=64 if name == "wrapping" else 1 << 24)
        Q.build(m, steps)
        for k, (cloud, R, t) in enumerate(asks):
            poses = S.faces_poses() if name == "faces" else np.concatenate([S.rows_of([(R, t)]), S.pose_set(9, k)])
            for reach in (0, 1):
                for stride in (1, 3):
                    S.hold(m, cloud, poses, reach, 0.3, stride, (name, kind, k, reach, stride))


def test_host_score_faces_poses_keep_points_on_faces():
    cloud = Q.faces()[1][0][0]
    finite = cloud[np.all(np.isfinite(cloud), axis=1) & np.all(np.abs(cloud) < 100.0, axis=1)]
    q = E.positions(finite, np.eye(3), S.faces_poses()[1, 9:])
    assert np.count_nonzero(np.all(q / Q.VOXEL == np.floor(q / Q.VOXEL), axis=1)) > 100


def test_host_score_nonfinite_points(twin):
    m = twin("plain")
    Q.build(m, Q.dense_map())
    cloud = E.with_nonfinite(Q.sized_cloud(257), 9)
    got = S.hold(m, cloud, S.pose_set(5), 1, np.inf, 1, "nonfinite")
    assert got[0, 0] == int(np.count_nonzero(np.all(np.isfinite(cloud), axis=1))) < 257


def test_host_score_of_one_pose_is_the_scoring_query(twin):
    for kind in KINDS:
        m = twin(kind)
        Q.build(m, Q.dense_map())
        cloud = Q.sized_cloud(257)
        for reach in (0, 1):
            R, t = Q.MAP_POSE
            got = S.call(m, cloud, S.rows_of([(R, t)]), reach, 0.3, 1)
            assert got.shape == (1, 3) and tuple(int(v) for v in got[0]) == tuple(m.query(cloud, R, t, reach, 0.3, False))


def test_host_score_accepts_4x4_poses(twin):
    m = twin("plain")
    Q.build(m, Q.dense_map())
    rows = S.pose_set(5)
    T = np.tile(np.eye(4), (5, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = rows[:, :9].reshape(5, 3, 3), rows[:, 9:]
    assert np.array_equal(m.map.score(Q.sized_cloud(65), T), m.map.score(Q.sized_cloud(65), rows))
    with pytest.raises(ValueError):
        m.map.score(Q.sized_cloud(65), np.zeros((5, 3, 4)))


def _raw(h, cloud, n, poses, K, reach, max_dist, stride, counts):
    p = lambda a, ct: None if a is None else a.ctypes.data_as(ct)
    dp = C.POINTER(C.c_double)
    return capi.host_lib().madicp_host_map_score(h, p(cloud, dp), n, p(poses, dp), K, reach, max_dist, stride, p(counts, C.POINTER(C.c_uint64)))


def test_host_score_refusals_write_nothing(twin):
    m = twin("plain")
    cloud = np.ascontiguousarray(E.gaussian(40, 1))
    m.insert(cloud, *E.IDENTITY, None)
    K = 6
    poses = S.pose_set(K)

    def refused(h=None, cloud_=cloud, n=40, poses_=poses, K_=K, reach=1, max_dist=1.0, stride=1, with_counts=True):
        counts = np.full(3 * S.CHUNK * 2, S.SENTINEL, np.uint64)
        assert _raw(m.h if h is None else h, cloud_, n, poses_, K_, reach, max_dist, stride, counts if with_counts else None) == INVALID
        assert np.all(counts == S.SENTINEL)

    refused(h=C.c_void_p())
    refused(poses_=None)
    refused(with_counts=False)
    refused(cloud_=None)
    refused(n=-1)
    for K_ in (0, -1, 4097):
        refused(poses_=np.tile(poses[0], (4097, 1)), K_=K_)
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 12 * (K - 1) + 11, 12 * (K - 1) + 4):  # (the first entry, t of the last pose, R of the last pose)
            P = poses.copy()
            P.reshape(-1)[at] = bad
            refused(poses_=P)
    for reach in (-1, 2, 27):
        refused(reach=reach)
    for max_dist in (np.nan, -1.0, -np.inf):
        refused(max_dist=max_dist)
    for stride in (0, -1, -(1 << 62)):
        refused(stride=stride)
    counts = np.full(3 * K + 3, S.SENTINEL, np.uint64)
    assert _raw(m.h, None, 0, poses, K, 1, 0.0, 1, counts) == 0  # n = 0 is legal here: zeros, and nothing behind the K rows
    assert np.all(counts[:3 * K] == 0) and np.all(counts[3 * K:] == S.SENTINEL)
    counts = np.full(3 * K + 3, S.SENTINEL, np.uint64)
    assert _raw(m.h, cloud, 40, poses, K, 1, np.inf, 1 << 62, counts) == 0  # a stride beyond the cloud: its first point alone
    assert counts[0] == 1 and np.all(counts[3 * K:] == S.SENTINEL)
