"""Pipeline.mapState / mapMergeRows and mad_icp_amd.map_io where no device is needed: the host front-end.

A Pipeline folds frames only behind compute(), which registers on the device, so the maps here come from capi.HostMap — the host
twin that stands behind the host front-end — and enter a Pipeline the way a saved map does: through mapMergeRows before its first
frame.  From there on everything is Pipeline's own: mapState of one pipeline merged into a second, save_map / load_map through a
file, a spec that does not match, mapNewRows that reports the merged rows once, a MapMirror fed across a merge, and the
relocalisation scene of tests/test_pipeline_map_score.py, whose mapRelocalize answers are the same bits in a fresh pipeline that
loaded the saved file.  tests/test_gpu_pipeline_map_merge.py drives frames on both front-ends."""
import numpy as np
import pytest

import cloud_export_ref as E
import map_merge_ref as G
import map_score_ref as S
from mad_icp_amd import capi, map_io
from mad_icp_amd.map_mirror import MapMirror
from test_pipeline_map_score import ALIGN, pipeline  # noqa: F401 (pipeline is a fixture)

EVIDENCE = (2, 1, 6)
STATE_COLUMNS = ("keys", "rows", "attribute", "evidence_words", "moment_words")


def state_bytes(st):
    return [(name, None if st[name] is None else (st[name].dtype.str, st[name].shape, st[name].tobytes())) for name in STATE_COLUMNS] + [
        (name, st[name]) for name in ("voxel", "with_attribute", "evidence", "moments")]


def twin_columns(voxel, with_attr, evidence, max_count, clouds):
    """the columns of a host twin that folded `clouds` (cloud, R, t[, words]) — what a Pipeline's host front-end would hold"""
    h = capi.HostMap.create(voxel, 64, 1 << 22, with_attr, evidence, max_count)
    try:
        for cloud, R, t, *words in clouds:
            h.insert(cloud, R, t, *(words if with_attr else ()))
        rows, keys, *w = h.download_rows(with_keys=True, with_attr=with_attr)
        return dict(keys=keys, rows=rows, attribute=w[0] if with_attr else None, evidence=h.download_evidence() if evidence else None,
                    moments=h.download_moments() if max_count else None)
    finally:
        h.close()


def full_map(pipeline_, front=False):
    """a pipeline with every column, its map merged in from a twin's"""
    p = pipeline_(front)
    p.setMapAccumulation(0.25, with_attribute=True, evidence=EVIDENCE, moments=4)
    clouds = [(E.gaussian(1500, 3 + i, scale=2.0), *E.IDENTITY, np.arange(1500, dtype=np.uint32) * 7 + i) for i in range(2)]
    cols = twin_columns(0.25, True, EVIDENCE, 4, clouds)
    return p, cols


def test_state_of_one_pipeline_merges_into_a_second_before_its_first_frame(pipeline):
    p, cols = full_map(pipeline)
    n = cols["keys"].shape[0]
    empty = p.mapState()
    assert empty["keys"].shape == (0,) and empty["rows"].shape == (0, 3) and empty["moment_words"].shape == (0, 10) and empty["evidence"] == EVIDENCE
    assert p.mapMergeRows(**cols) == (n, n) and p.mapSize() == n > 1000
    st = p.mapState()
    assert (st["voxel"], st["with_attribute"], st["evidence"], st["moments"]) == (0.25, True, EVIDENCE, 4)
    for name, col in zip(STATE_COLUMNS, ("keys", "rows", "attribute", "evidence", "moments")):
        assert st[name].dtype == cols[col].dtype and st[name].tobytes() == cols[col].tobytes(), name
    assert st["attribute"].dtype == np.uint32  # (the words travel as uint32)
    q = pipeline()
    q.setMapAccumulation(0.25, with_attribute=True, evidence=EVIDENCE, moments=4)
    assert q.mapMergeRows(st["keys"], st["rows"], st["attribute"], st["evidence_words"], st["moment_words"]) == (n, n)
    assert state_bytes(q.mapState()) == state_bytes(st)
    assert [c.tobytes() for c in q.mapSurfels()] == [c.tobytes() for c in p.mapSurfels()]
    # a second merge of the same rows: no row added, evidence saturating, the open rows' moments doubled
    assert q.mapMergeRows(st["keys"], st["rows"], st["attribute"], st["evidence_words"], st["moment_words"]) == (0, n)
    want, _ = G.merge(dict(keys=st["keys"], xyz=st["rows"], attr=st["attribute"], evidence=st["evidence_words"], moments=st["moment_words"]),
                      dict(keys=st["keys"], xyz=st["rows"], attr=st["attribute"], evidence=st["evidence_words"], moments=st["moment_words"]),
                      dict(with_attr=True, evidence=EVIDENCE, max_count=4))
    again = q.mapState()
    assert again["evidence_words"].tobytes() == want["evidence"].tobytes() and again["moment_words"].tobytes() == want["moments"].tobytes()
    assert again["rows"].tobytes() == st["rows"].tobytes() and again["moment_words"].tobytes() != st["moment_words"].tobytes()


def test_a_float_attribute_is_taken_by_its_bits(pipeline):
    p = pipeline()
    p.setMapAccumulation(0.25, with_attribute=True)
    keys = G.distinct_keys(4, 1)
    rows = np.zeros((4, 3), np.float32)
    words = np.array([0x7fc00001, 0x80000000, 0x3f800000, 0xffc12345], np.uint32)
    assert p.mapMergeRows(keys, rows, words.view(np.float32)) == (4, 4)
    assert p.mapState()["attribute"].tobytes() == words.tobytes()
    with pytest.raises(ValueError):
        p.mapMergeRows(G.distinct_keys(4, 2), rows, words.astype(np.float64))


def test_save_and_load_through_a_file(pipeline, tmp_path):
    p, cols = full_map(pipeline)
    p.mapMergeRows(**cols)
    path = str(tmp_path / "map.npz")
    assert map_io.save_map(p, path) == p.mapSize()
    with np.load(path, allow_pickle=False) as f:
        assert set(f.files) == {"format", "voxel", "with_attribute", "evidence", "moments", "keys", "rows", "attribute", "evidence_words", "moment_words"}
    q = pipeline()
    q.setMapAccumulation(0.25, with_attribute=True, evidence=EVIDENCE, moments=4)
    assert map_io.load_map(q, path) == (p.mapSize(), p.mapSize())
    assert state_bytes(q.mapState()) == state_bytes(p.mapState())
    plain = pipeline()
    plain.setMapAccumulation(0.25)
    plain.mapMergeRows(cols["keys"], cols["rows"])
    path2 = str(tmp_path / "plain.npz")
    map_io.save_map(plain, path2)
    with np.load(path2, allow_pickle=False) as f:
        assert set(f.files) == {"format", "voxel", "with_attribute", "evidence", "moments", "keys", "rows"}
    back = pipeline()
    back.setMapAccumulation(0.25)
    assert map_io.load_map(back, path2) == (plain.mapSize(), plain.mapSize()) and state_bytes(back.mapState()) == state_bytes(plain.mapState())


def test_a_spec_that_does_not_match_raises(pipeline, tmp_path):
    p, cols = full_map(pipeline)
    p.mapMergeRows(**cols)
    path = str(tmp_path / "map.npz")
    map_io.save_map(p, path)
    for kw, word in ((dict(voxel_size=0.5, with_attribute=True, evidence=EVIDENCE, moments=4), "voxel"),
                     (dict(voxel_size=0.25, evidence=EVIDENCE, moments=4), "attribute"),
                     (dict(voxel_size=0.25, with_attribute=True, moments=4), "evidence"),
                     (dict(voxel_size=0.25, with_attribute=True, evidence=EVIDENCE), "moments")):
        q = pipeline()
        q.setMapAccumulation(**kw)
        with pytest.raises(ValueError, match=word):
            map_io.load_map(q, path)
        assert q.mapSize() == 0
    off = pipeline()
    with pytest.raises(ValueError):
        map_io.load_map(off, path)
    with pytest.raises(RuntimeError):
        off.mapState()
    with pytest.raises(RuntimeError):
        off.mapMergeRows(cols["keys"], cols["rows"])
    # the calls' own refusals: a column the map lacks or misses, unequal lengths, a key with bit 63, evidence 0
    q = pipeline()
    q.setMapAccumulation(0.25, evidence=EVIDENCE)
    k, r, e = cols["keys"][:5], cols["rows"][:5], np.ones(5, np.uint32)
    for args in ((k, r), (k, r, np.zeros(5, np.uint32), e), (k, r, None, e, np.ones((5, 10), np.uint64)), (k, r[:4], None, e), (k, r, None, e[:4]),
                 (k | np.uint64(1 << 63), r, None, e), (k, r, None, e * 0), (k, r.astype(np.float64), None, e)):
        with pytest.raises((ValueError, TypeError)):
            q.mapMergeRows(*args)
        assert q.mapSize() == 0
    assert q.mapMergeRows(k, r, None, e) == (5, 5)


def test_a_capacity_refusal_throws_and_leaves_everything(pipeline):
    p = pipeline()
    p.setMapAccumulation(0.25, max_points=10)
    keys, rows = G.distinct_keys(11, 5), np.ones((11, 3), np.float32)
    with pytest.raises(RuntimeError):
        p.mapMergeRows(keys, rows)
    assert p.mapSize() == 0 and not p.mapOverflowed() and p.mapNewRows().shape == (0, 3)
    assert p.mapMergeRows(keys[:6], rows[:6]) == (6, 6)
    with pytest.raises(RuntimeError):
        p.mapMergeRows(keys[:5], rows[:5])  # (6 + 5 > 10, though every key is held: the fold's conservative rule)
    assert p.mapSize() == 6 and not p.mapOverflowed()
    assert p.mapMergeRows(keys[4:8], rows[4:8]) == (2, 8)


def test_new_rows_reports_the_merged_rows_once(pipeline):
    p, cols = full_map(pipeline)
    n = cols["keys"].shape[0]
    half = n // 2
    first = {k: (v[:half] if v is not None else None) for k, v in cols.items()}
    p.mapMergeRows(**first)
    rows, words, keys = p.mapNewRows(with_attribute=True, with_keys=True)
    assert rows.tobytes() == cols["rows"][:half].tobytes() and keys.tobytes() == cols["keys"][:half].tobytes()
    assert np.asarray(words).tobytes() == cols["attribute"][:half].tobytes()
    assert p.mapNewRows().shape == (0, 3)
    p.mapMergeRows(**cols)  # (the first half again, and the rest)
    rows, keys = p.mapNewRows(with_keys=True)
    assert rows.tobytes() == cols["rows"][half:].tobytes() and keys.tobytes() == cols["keys"][half:].tobytes()
    assert p.mapNewRows().shape == (0, 3) and p.mapSize() == n


def test_a_mirror_fed_across_a_merge_still_equals_the_map(pipeline):
    p, cols = full_map(pipeline)
    p.setMapTrackRemoved(True)
    mirror = MapMirror(with_attribute=True)
    n = cols["keys"].shape[0]
    third = {k: v[: n // 3] for k, v in cols.items()}
    p.mapMergeRows(**third)
    assert mirror.update(p) == (0, n // 3)
    removed = p.mapPrune(np.zeros(3), 2.0)  # (rows the mirror holds leave; the log tells it)
    assert removed > 0
    p.mapMergeRows(**cols)  # (some of the pruned voxels come back as new rows)
    assert mirror.update(p) == (removed, n - n // 3 + removed)
    order = np.argsort(p.mapKeys(), kind="stable")
    assert mirror.keys().tobytes() == p.mapKeys()[order].tobytes() and mirror.rows().tobytes() == p.mapCloud()[order].tobytes()
    assert mirror.attr().tobytes() == p.mapState()["attribute"][order].tobytes() and len(mirror) == p.mapSize() == n


def test_the_scene_relocalises_the_same_from_a_saved_file(pipeline, tmp_path):
    sc = S.scene()
    cols = twin_columns(S.SCENE_VOXEL, False, None, 1 << 20, [(scan, T[:3, :3], T[:3, 3]) for scan, T in zip(sc["scans"][:-1], sc["poses"])])
    cloud, hyp, index = sc["scans"][-1], sc["hypotheses"], sc["index"]
    p = pipeline()
    p.setMapAccumulation(S.SCENE_VOXEL, moments=1 << 20)
    p.mapMergeRows(cols["keys"], cols["rows"], moments=cols["moments"])
    want = p.mapRelocalize(cloud, hyp, refine=4, iterations=10, stride=8, **ALIGN)
    assert want["index"][0] == index and want["best"] == 0
    path = str(tmp_path / "scene.npz")
    map_io.save_map(p, path)
    del p  # (the restart)
    q = pipeline()
    q.setMapAccumulation(S.SCENE_VOXEL, moments=1 << 20)
    map_io.load_map(q, path)
    got = q.mapRelocalize(cloud, hyp, refine=4, iterations=10, stride=8, **ALIGN)
    for name in ("index", "scores", "poses", "H", "b", "chi2", "counts"):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    assert got["best"] == want["best"]
    assert np.array_equal(q.mapScorePoses(cloud, hyp, 1, S.SCENE_MAX_DIST, 8),
                          S.score(cols["rows"], cols["keys"], cloud, capi.pose_rows(hyp), S.SCENE_VOXEL, 1, S.SCENE_MAX_DIST, 8))
