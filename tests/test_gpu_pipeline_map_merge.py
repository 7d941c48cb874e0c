"""Pipeline.mapState / mapMergeRows / map_io on both front-ends, with maps that frames made: the relocalisation scene of
tests/map_score_ref.py driven behind compute(), its map taken out and put into a fresh pipeline before that pipeline's first frame
— directly and through a saved file, on the same front-end and across (a device map restored from a host-twin save, and the
reverse).  The restored map is the map: every column the same bytes, mapRelocalize the same bits as the pipeline that drove, and
the first fold of the fresh pipeline finds it and goes on from it — the same on both front-ends."""
import numpy as np
import pytest

import map_score_ref as S
from mad_icp_amd import map_io
from test_gpu_pipeline_registered_scan import pipeline
from test_pipeline_map_merge import state_bytes
from test_pipeline_map_score import ALIGN

pytestmark = pytest.mark.gpu

SPEC = dict(evidence=(2, 1, 6), moments=1 << 20)


def fresh(device_frontend):
    p = pipeline(False, device_frontend)
    p.setMapAccumulation(S.SCENE_VOXEL, **SPEC)
    return p


@pytest.fixture(scope="module")
def fronts(natives):
    out = {}
    for front in (True, False):
        p = fresh(front)
        for i, scan in enumerate(S.scene()["scans"][:-1]):
            p.compute(0.1 * i, scan)
        out[front] = p
    return out


def relocalised(p):
    sc = S.scene()
    got = p.mapRelocalize(sc["scans"][-1], sc["hypotheses"], refine=4, iterations=10, stride=8, **ALIGN)
    return [(name, got[name].tobytes() if name != "best" else got[name]) for name in ("index", "scores", "poses", "H", "b", "chi2", "counts", "best")]


def test_both_front_ends_drove_the_same_map(fronts):
    assert state_bytes(fronts[True].mapState()) == state_bytes(fronts[False].mapState()) and fronts[True].mapSize() > 1000


@pytest.mark.parametrize("saved_on", [True, False])
@pytest.mark.parametrize("restored_on", [True, False])
def test_a_saved_map_restores_on_either_front_end(fronts, tmp_path, saved_on, restored_on):
    src = fronts[saved_on]
    st = src.mapState()
    n = src.mapSize()
    path = str(tmp_path / "map.npz")
    assert map_io.save_map(src, path) == n
    direct, loaded = fresh(restored_on), fresh(restored_on)
    assert direct.mapMergeRows(st["keys"], st["rows"], None, st["evidence_words"], st["moment_words"]) == (n, n)
    assert map_io.load_map(loaded, path) == (n, n)
    for q in (direct, loaded):
        assert state_bytes(q.mapState()) == state_bytes(st)
        assert q.mapNewRows().tobytes() == st["rows"].tobytes() and q.mapNewRows().shape == (0, 3)  # new rows to a consumer, once
    # the same bits as the pipeline that drove on the front-end that answers (the registration's last bits belong to the side)
    assert relocalised(loaded) == relocalised(fronts[restored_on])
    assert relocalised(loaded)[0][1] == relocalised(src)[0][1] and relocalised(loaded)[1][1] == relocalised(src)[1][1]  # ranking and scores: everywhere


def test_the_first_fold_finds_the_restored_map(fronts, tmp_path):
    sc = S.scene()
    path = str(tmp_path / "map.npz")
    map_io.save_map(fronts[False], path)
    n = fronts[False].mapSize()
    after = {}
    for front in (True, False):
        q = fresh(front)
        map_io.load_map(q, path)
        q.compute(0.0, sc["scans"][0])  # (the first frame of a pipeline stands at the identity: the scene's first pose)
        assert q.mapSize() >= n and q.mapNewRows().shape[0] == q.mapSize()
        after[front] = q.mapState()
        # the restored rows stand where they stood; the fold hit them (evidence) and added to their moments
        assert after[front]["keys"][:n].tobytes() == fronts[False].mapState()["keys"].tobytes()
        assert after[front]["moment_words"][:n, 0].sum() > fronts[False].mapState()["moment_words"][:, 0].sum()
    assert state_bytes(after[True]) == state_bytes(after[False])


def test_a_merge_into_a_driven_map_is_one_fold_on_both_front_ends(fronts):
    """the map of the other front-end merged into a copy of one's own: every key present, evidence saturating, moments doubled"""
    out = {}
    for front in (True, False):
        q = fresh(front)
        st = fronts[front].mapState()
        n = st["keys"].shape[0]
        q.mapMergeRows(st["keys"], st["rows"], None, st["evidence_words"], st["moment_words"])
        other = fronts[not front].mapState()
        assert q.mapMergeRows(other["keys"], other["rows"], None, other["evidence_words"], other["moment_words"]) == (0, n)
        out[front] = q.mapState()
        assert np.array_equal(out[front]["moment_words"], 2 * st["moment_words"])
        assert np.array_equal(out[front]["evidence_words"], np.minimum(2 * st["evidence_words"].astype(np.int64), 6))
    assert state_bytes(out[True]) == state_bytes(out[False])
