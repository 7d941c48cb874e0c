"""Pipeline.mapScorePoses / mapRelocalize on the relocalisation scene of tests/map_score_ref.py, device front-end against host
front-end: a few frames folded behind compute(), the next scan, a pose grid of which one element stands by the scan's true pose.
On each front-end the scores are the restatement over the map's own rows and keys and mapRelocalize is its composition bit for
bit; between the front-ends scores and ranking are equal, registered poses within the project's bound for mapRegister device
against twin (1e-5 m / 1e-5 rad), closing counts equal at the first refined hypothesis; the good hypothesis ranks first, is best
and ends nearer the truth than it began.  And a drive that calls mapScorePoses between frames is bit for bit the drive that does
not."""
import numpy as np
import pytest

import map_score_ref as S
from mad_icp_amd import capi
from test_gpu_pipeline_registered_scan import bits, pipeline
from test_pipeline_map_score import ALIGN, composition, same_relocalisation

pytestmark = pytest.mark.gpu


def everything(p):
    return [c.tobytes() for c in (p.mapCloud(), p.mapKeys(), p.mapMoments()) + tuple(p.mapSurfels())]


def driven(device_frontend, between=None):
    sc = S.scene()
    p = pipeline(False, device_frontend)
    p.setMapAccumulation(S.SCENE_VOXEL, moments=1 << 20)
    for i, scan in enumerate(sc["scans"][:-1]):
        p.compute(0.1 * i, scan)
        if between:
            between(p)
    return p


@pytest.fixture(scope="module")
def fronts(natives):
    return {front: driven(front) for front in (True, False)}


@pytest.mark.parametrize("device_frontend", [True, False])
def test_scores_are_the_restatement_and_relocalize_is_its_composition(fronts, device_frontend):
    sc = S.scene()
    p = fronts[device_frontend]
    cloud, G, index = sc["scans"][-1], sc["hypotheses"], sc["index"]
    before, pose = everything(p), bits(np.asarray(p.currentPose()))
    rows, keys = p.mapCloud(), p.mapKeys()
    for reach, stride in ((1, 1), (0, 8), (1, 8)):
        got = p.mapScorePoses(cloud, G, reach, S.SCENE_MAX_DIST, stride)
        assert np.array_equal(got, S.score(rows, keys, cloud, capi.pose_rows(G), S.SCENE_VOXEL, reach, S.SCENE_MAX_DIST, stride)), (reach, stride)
        order = S.rank(got)
        assert order[0] == index and got[order[0], 2] > got[order[1], 2], (reach, stride, order[:3], got[order[:3]])
    got = p.mapRelocalize(cloud, G, refine=4, iterations=10, stride=8, **ALIGN)
    same_relocalisation(got, composition(p, cloud, G, 4, 10, 8, **ALIGN))
    assert got["index"][0] == index and got["best"] == 0
    start, end = S.pose_distance(sc["truth"], G[index]), S.pose_distance(sc["truth"], got["poses"][0])
    assert end[0] <= start[0] and end[1] <= start[1], (start, end)
    assert everything(p) == before and np.array_equal(bits(np.asarray(p.currentPose())), pose)  # only read, the pose not touched


def test_device_front_end_against_host_front_end(fronts):
    sc = S.scene()
    cloud, G = sc["scans"][-1], sc["hypotheses"]
    d, h = fronts[True], fronts[False]
    assert everything(d)[:3] == everything(h)[:3]  # (rows, keys and moments: the same map)
    for reach, stride in ((1, 1), (0, 8), (1, 8)):
        assert np.array_equal(d.mapScorePoses(cloud, G, reach, S.SCENE_MAX_DIST, stride), h.mapScorePoses(cloud, G, reach, S.SCENE_MAX_DIST, stride))
    a, b = (p.mapRelocalize(cloud, G, refine=4, iterations=10, stride=8, **ALIGN) for p in (d, h))
    assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["scores"], b["scores"]) and a["best"] == b["best"]
    for r in range(4):
        dt, da = S.pose_distance(a["poses"][r], b["poses"][r])
        assert dt <= 1e-5 and da <= 1e-5, (r, dt, da)
    assert np.array_equal(a["counts"][0], b["counts"][0])


@pytest.mark.parametrize("device_frontend", [True, False])
def test_calling_it_between_frames_changes_nothing(fronts, device_frontend):
    sc = S.scene()
    asked = []
    with_calls = driven(device_frontend, lambda p: asked.append(p.mapScorePoses(sc["scans"][-1], sc["hypotheses"][:70], 1, S.SCENE_MAX_DIST, 8)))
    without = fronts[device_frontend]
    assert len(asked) == S.SCENE_FRAMES and asked[-1][:, 1].any()
    assert np.array_equal(bits(np.asarray(with_calls.trajectory())), bits(np.asarray(without.trajectory())))
    assert everything(with_calls) == everything(without)
