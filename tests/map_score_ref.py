"""Scoring many poses (include/madicp_hip.h: madicp_map_score_poses) restated over the map query's restatement, and what the host
and the device tests share.  The restatement is the definition read literally: for each pose k the counts of
map_query_ref.query(rows, keys, cloud[::stride], R_k, t_k, ...) — K separate queries of the subsampled cloud.  It is computed
once per (rows, keys, cloud, poses, reach, max_dist, stride) and shared by every test that asks for it again."""
import numpy as np

import cloud_export_ref as E
import map_query_ref as Q

VOXEL = Q.VOXEL
CHUNK = 64  # the kernel's pose chunk (fe::kScoreChunk): the K sets below stand around it
CLOUD_SIZES = [0, 1, 63, 64, 65, 257, 1025]
POSE_COUNTS = [1, 2, 63, 64, 65, 130]
MAX_DISTS = [0.0, 0.3, np.inf]
SENTINEL = np.uint64(0x7777777777777777)

_seen = {}


def rows_of(poses):
    """(K, 12) float64: R row-major, then t — from a list of (R, t)"""
    return np.ascontiguousarray([np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]) for R, t in poses])


def score(rows, keys, cloud, poses, voxel=VOXEL, reach=1, max_dist=np.inf, stride=1):
    """(K, 3) uint64: the restatement"""
    cloud = np.ascontiguousarray(cloud, np.float64).reshape(-1, 3)
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    at = (np.asarray(rows).tobytes(), np.asarray(keys).tobytes(), cloud.tobytes(), poses.tobytes(), voxel, reach, float(max_dist), int(stride))
    if at not in _seen:
        sub = cloud[::stride]
        _seen[at] = np.array([Q.query(rows, keys, sub, X[:9].reshape(3, 3), X[9:], voxel, reach, max_dist)["counts"] for X in poses],
                             np.uint64).reshape(-1, 3)
    return _seen[at]


def strides(n):
    return sorted({1, 2, 7, max(n, 1), n + 1})


def pose_set(K, seed=0):
    """K poses for a cloud seen through Q.MAP_POSE: that pose, the identity, a pose that throws every point outside the key range, a
    shift by whole voxels, small displacements of MAP_POSE — and, from K = 5 on, the last pose is the first again"""
    R, t = Q.MAP_POSE
    rng = np.random.default_rng(1000 + 7 * K + seed)
    poses = [(R, t), E.IDENTITY, (R, t + np.array([3e6, 0.0, 0.0])), (R, t + np.array([VOXEL, -2 * VOXEL, 3 * VOXEL]))]
    while len(poses) < K:
        dR, _ = E.random_pose(int(rng.integers(1 << 30)))
        w = rng.uniform(0.0, 1.0)
        poses.append((R if w < 0.5 else dR @ R, t + rng.normal(size=3) * 0.4))
    poses = poses[:K]
    if K >= 5:
        poses[-1] = poses[0]
    return rows_of(poses)


def combos(n):
    """(K, stride, reach, max_dist) for a cloud of n points: every K at rotating settings, then K = 3 at every setting"""
    S = strides(n)
    out = [(K, S[i % len(S)], i % 2, MAX_DISTS[i % 3]) for i, K in enumerate(POSE_COUNTS)]
    out += [(3, s, reach, md) for s in S for reach in (0, 1) for md in MAX_DISTS]
    return out


def call(impl, cloud, poses, reach=1, max_dist=np.inf, stride=1):
    """impl (tests/map_impls.py) asked: the host twin takes the points, the device map a resident cloud"""
    if hasattr(impl, "resident"):
        with impl.resident(cloud) as cid:
            return impl.map.score(cid, poses, reach, max_dist, stride)
    return impl.map.score(cloud, poses, reach, max_dist, stride)


def hold(impl, cloud, poses, reach, max_dist, stride, tag, voxel=VOXEL):
    """impl's answer against the restatement over impl's own stored rows; returns it"""
    want = score(impl.rows(), impl.keys(), cloud, poses, voxel, reach, max_dist, stride)
    got = call(impl, cloud, poses, reach, max_dist, stride)
    assert got.dtype == np.uint64 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (tag, np.nonzero(np.any(got != want, axis=1))[0][:8], got[:4], want[:4])
    return got


def faces_poses():
    """for Q.faces(): the identity and shifts by whole voxels (the points stay exactly on faces), one of them twice, and a pose
    that leaves the key range"""
    I = np.eye(3)
    shifts = [np.zeros(3), np.array([VOXEL, 0.0, 0.0]), np.array([-VOXEL, 2 * VOXEL, 0.0]), np.array([0.0, 0.0, -3 * VOXEL]), np.array([VOXEL, 0.0, 0.0]),
              np.array([0.0, 4e6, 0.0])]
    return rows_of([(I, s) for s in shifts])


# ---- the relocalisation scene (tests/test_pipeline_map_score.py on the host twin, tests/test_gpu_pipeline_map_score.py through
# Pipeline on both front-ends): a street of mad_icp_amd.synth dense enough in boxes that a shift along it changes the score -------
SCENE_VOXEL, SCENE_MAX_DIST, SCENE_FRAMES = 0.5, 0.25, 4
SCENE_NUDGE = (0.10, 0.5)  # metres, degrees: how far the one good hypothesis stands from the scan's true pose


def rank(counts):
    """the hypotheses by (within descending, index ascending)"""
    within = np.asarray(counts)[:, 2].astype(np.int64)
    return np.lexsort((np.arange(within.shape[0]), -within))


def pose_distance(A, B):
    D = np.linalg.inv(A) @ B
    return float(np.linalg.norm(D[:3, 3])), float(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


def scene():
    """dict(scans: SCENE_FRAMES + 1 scans of 16 x 450 rays, poses: their true poses in the first scan's frame, truth: the last
    one's, hypotheses (125, 4, 4): mad_icp_amd.relocalize.pose_grid around a centre one step behind, of which element `index` is
    the truth nudged by SCENE_NUDGE — inside the registration's basin — and every other one at least two voxels or 20 degrees
    from it)"""
    if "scene" not in _seen:
        from mad_icp_amd import synth
        from mad_icp_amd.relocalize import pose_grid

        world = synth.Scene(1, n_boxes=200)
        P = [synth.path_pose(1.0 * i) for i in range(SCENE_FRAMES + 1)]
        scans = [np.ascontiguousarray(synth.render_scan(world, P[i], 100 + i, n_beams=16, n_azimuth=450), np.float64) for i in range(len(P))]
        poses = [np.linalg.inv(P[0]) @ p for p in P]
        truth = poses[-1]
        good = truth @ synth.perturbation(5, trans=SCENE_NUDGE[0], rot_deg=SCENE_NUDGE[1])
        step = np.eye(4)
        step[0, 3] = 2 * SCENE_VOXEL
        G = pose_grid(good @ np.linalg.inv(step), 4 * SCENE_VOXEL, 2 * SCENE_VOXEL, np.deg2rad(40.0), 2)
        near = [k for k in range(G.shape[0]) if np.allclose(G[k], good, atol=1e-9)]
        assert len(near) == 1 and near[0] != 0
        G[near[0]] = good
        for k in range(G.shape[0]):
            dt, da = pose_distance(good, G[k])
            assert k == near[0] or dt >= 2 * SCENE_VOXEL - 1e-9 or da >= np.deg2rad(20.0) - 1e-9, (k, dt, da)
        _seen["scene"] = dict(scans=scans, poses=poses, truth=truth, hypotheses=G, index=near[0])
    return _seen["scene"]
