"""Pipeline.mapScorePoses / mapRelocalize where no device is needed, and the relocalisation scene on the host twin alone.

A Pipeline folds frames only behind compute(), which registers on the device: what a Pipeline can be asked here is everything in
front of the first fold — the errors, and the empty map, where mapScorePoses is the restatement over no rows and mapRelocalize is
its own composition (mapScorePoses -> rank -> mapRegister) bit for bit.  The scene of tests/map_score_ref.py — a few frames folded,
the next scan, a pose grid of which one element stands by the scan's true pose — is held here on capi.HostMap, the host twin
behind the host front-end: that element ranks first, is `best`, and its registration ends nearer the truth than it began.
tests/test_gpu_pipeline_map_score.py drives the same scene through Pipeline on both front-ends."""
import numpy as np
import pytest

import map_score_ref as S
from fixtures import B_MAX, B_MIN, B_RATIO, RHO_KER
from mad_icp_amd import capi

ALIGN = dict(reach=1, max_dist=S.SCENE_MAX_DIST, rho=float("inf"), min_count=3, flat=1.0)


@pytest.fixture
def pipeline(natives):
    from mad_icp.src.pybind import pypeline as m

    def make(device_frontend=False):
        p = m.Pipeline(10.0, False, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, 4, 4, False)
        p.setDeviceFrontEnd(device_frontend)
        return p

    return make


def composition(p, cloud, poses, refine, iterations, stride, **align):
    """mapRelocalize spelled out over the calls it is made of"""
    counts = p.mapScorePoses(cloud, poses, align["reach"], align["max_dist"], stride)
    order = S.rank(counts)[:refine]
    out = dict(index=order.astype(np.int32), scores=counts[order], poses=[], H=[], b=[], chi2=[], counts=[])
    for k in order:
        pose, info = p.mapRegister(cloud, poses[k], iterations, **align)
        out["poses"].append(pose)
        for name in ("H", "b", "chi2", "counts"):
            out[name].append(info[name])
    inliers = [int(c[3]) for c in out["counts"]]
    out["best"] = inliers.index(max(inliers))
    return out


def same_relocalisation(got, want):
    assert got["index"].dtype == np.int32 and np.array_equal(got["index"], want["index"])
    assert got["scores"].dtype == np.uint64 and np.array_equal(got["scores"], want["scores"])
    for name in ("poses", "H", "b", "chi2", "counts"):
        w = np.asarray(want[name])
        assert got[name].shape == w.shape and got[name].tobytes() == w.astype(got[name].dtype).tobytes(), name
    assert got["best"] == want["best"]


def test_errors_by_exception_type(pipeline):
    sc = S.scene()
    cloud, G = sc["scans"][-1][:200], sc["hypotheses"]
    for front in (False, True):
        p = pipeline(front)
        with pytest.raises(RuntimeError):
            p.mapScorePoses(cloud, G)  # accumulation is off
        with pytest.raises(RuntimeError):
            p.mapRelocalize(cloud, G)
        p.setMapAccumulation(S.SCENE_VOXEL)
        with pytest.raises(RuntimeError):
            p.mapRelocalize(cloud, G)  # no moments
        assert p.mapScorePoses(cloud, G).shape == (125, 3)  # (scoring needs none)
        p.setMapAccumulation(S.SCENE_VOXEL, moments=1 << 20)
        for refine in (0, -1, 65):
            with pytest.raises(ValueError):
                p.mapRelocalize(cloud, G, refine=refine)
        bad = G.copy()
        bad[-1, 2, 3] = np.nan  # (one entry of the LAST pose refuses the whole call)
        for kw in (dict(poses=bad), dict(poses=G[:0]), dict(poses=np.tile(G[:1], (4097, 1, 1))), dict(poses=G[:, :3]), dict(reach=2), dict(reach=-1),
                   dict(max_dist=-1.0), dict(max_dist=np.nan), dict(stride=0), dict(stride=-3), dict(cloud=cloud[:, :2])):
            args = dict(dict(cloud=cloud, poses=G), **kw)
            with pytest.raises(ValueError):
                p.mapScorePoses(**args)
            with pytest.raises(ValueError):
                p.mapRelocalize(**args)
        for kw in (dict(iterations=-1), dict(iterations=65), dict(rho=0.0), dict(min_count=2), dict(flat=0.0)):
            with pytest.raises(ValueError):
                p.mapRelocalize(cloud, G, **kw)


def test_before_the_first_fold_every_candidate_is_unmatched(pipeline):
    sc = S.scene()
    cloud, G = sc["scans"][-1], sc["hypotheses"]
    for front in (False, True):
        p = pipeline(front)
        p.setMapAccumulation(S.SCENE_VOXEL, moments=1 << 20)
        rows12 = capi.pose_rows(G)
        for reach, md, stride in ((1, np.inf, 1), (0, 0.25, 8), (1, 0.0, 7179)):
            got = p.mapScorePoses(cloud, G, reach, md, stride)
            want = S.score(np.zeros((0, 3), np.float32), np.zeros(0, np.uint64), cloud, rows12, S.SCENE_VOXEL, reach, md, stride)
            assert got.dtype == np.uint64 and np.array_equal(got, want) and not got[:, 1:].any() and got[:, 0].all()
            assert np.array_equal(p.mapScorePoses(cloud, rows12, reach, md, stride), got)  # (K, 12) is (K, 4, 4)
        assert np.array_equal(p.mapScorePoses(cloud[:0], G), np.zeros((125, 3), np.uint64))
        got = p.mapRelocalize(cloud, G, refine=3, iterations=2, stride=8, **ALIGN)
        same_relocalisation(got, composition(p, cloud, G, 3, 2, 8, **ALIGN))
        assert got["index"].tolist() == [0, 1, 2] and got["best"] == 0 and np.array_equal(got["poses"], G[:3])  # all tied: by index
        assert p.mapRelocalize(cloud, G[:2], refine=4, iterations=1)["index"].tolist() == [0, 1]  # min(refine, K)
        assert p.mapSize() == 0


class TwinPipeline:
    """the two calls of a Pipeline's host front-end that the composition is made of, on a capi.HostMap"""

    def __init__(self, h):
        self.h = h

    def mapScorePoses(self, cloud, poses, reach, max_dist, stride):
        return self.h.score(cloud, poses, reach, max_dist, stride)

    def mapRegister(self, cloud, pose, iterations, **align):
        r = self.h.register(cloud, pose[:3, :3], pose[:3, 3], iterations, **align)
        X = np.eye(4)
        X[:3, :3], X[:3, 3] = r["R"], r["t"]
        return X, dict(H=r["H"][-1], b=r["b"][-1], chi2=r["chi2"][-1], counts=r["counts"][-1])


def test_the_scene_relocalises_on_the_host_twin(natives):
    sc = S.scene()
    h = capi.HostMap.create(S.SCENE_VOXEL, 1 << 12, 1 << 22, False, None, 1 << 20)
    try:
        for scan, T in zip(sc["scans"][:-1], sc["poses"]):
            h.insert(scan, T[:3, :3], T[:3, 3])
        cloud, G, index = sc["scans"][-1], sc["hypotheses"], sc["index"]
        for stride in (1, 8):
            counts = h.score(cloud, G, 1, S.SCENE_MAX_DIST, stride)
            assert np.array_equal(counts, S.score(h.download_f32(), h.download_keys(), cloud, capi.pose_rows(G), S.SCENE_VOXEL, 1, S.SCENE_MAX_DIST,
                                                  stride))
            order = S.rank(counts)
            assert order[0] == index and counts[order[0], 2] > counts[order[1], 2], (stride, order[:3], counts[order[:3]])
        got = composition(TwinPipeline(h), cloud, G, 4, 10, 8, **ALIGN)
        assert got["index"][0] == index and got["best"] == 0
        before, after = S.pose_distance(sc["truth"], G[index]), S.pose_distance(sc["truth"], got["poses"][0])
        assert after[0] <= before[0] and after[1] <= before[1], (before, after)
    finally:
        h.close()
