"""Pipeline.mapQuery / mapOverlap / setMapOverlap — asking the voxel map where it lives — on the 8-frame 16 x 450 drive of
tests/test_gpu_pipeline_registered_scan.py, both front-ends: mapQuery and mapOverlap are the restatement of tests/map_query_ref.py
applied to mapCloud / mapKeys / mapEvidence of that moment; with setMapOverlap(True) every frame's mapFrameOverlap() is the
restatement applied to the map as it stood before that frame's fold (zeros for a frame keyframes_only skipped); poses, keyframe
decisions and every map column are the same bits with the option on and off; the errors.  Everything is exact equality."""
import numpy as np
import pytest

import map_query_ref as Q
from test_gpu_pipeline_registered_scan import bits, drive, feed, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
EVIDENCE = (2, 1, 6)
MAX_DIST = 0.3


def columns(p):
    if p.mapSize() == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    return p.mapCloud(), p.mapKeys(), p.mapEvidence() if p.mapWithEvidence() else np.zeros(0, np.uint32)


def counts_of(p, cloud, T, reach, max_dist):
    rows, keys, ev = columns(p)
    return Q.query(rows, keys, cloud, T[:3, :3], np.array(T[:3, 3]), VOXEL, reach, max_dist, ev=ev)["counts"]


@pytest.mark.parametrize("device_frontend", [True, False])
def test_drive_overlap_of_every_frame_and_the_same_bits(natives, drive, device_frontend):
    on, off, kf = pipeline(False, device_frontend), pipeline(False, device_frontend), pipeline(False, device_frontend)
    for p in (on, off):
        p.setMapAccumulation(VOXEL, evidence=EVIDENCE)
    kf.setMapAccumulation(VOXEL, True)
    on.setMapOverlap(True, 1, MAX_DIST)
    kf.setMapOverlap(True, 0)
    assert on.mapFrameOverlap() == (0, 0, 0) and off.mapFrameOverlap() == (0, 0, 0)
    skipped = matched = 0
    for i, f in enumerate(drive):
        before = columns(on), columns(kf)
        for p in (on, off, kf):
            feed(p, "cloud", i, f)
        for other in (off, kf):
            assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(other.currentPose()))), i
            assert on.keyframeID() == other.keyframeID() and on.isMapUpdated() == other.isMapUpdated(), i
        T = np.asarray(on.currentPose())
        R, t = T[:3, :3], np.array(T[:3, 3])
        want = Q.query(before[0][0], before[0][1], f["pts"], R, t, VOXEL, 1, MAX_DIST)["counts"]
        assert on.mapFrameOverlap() == want and off.mapFrameOverlap() == (0, 0, 0), (i, on.mapFrameOverlap(), want)
        assert want[0] == f["pts"].shape[0] > 6000 and (i == 0) == (want[1] == 0) and want[2] <= want[1] <= want[0], (i, want)
        matched += want[1]
        if kf.isMapUpdated():
            assert kf.mapFrameOverlap() == Q.query(before[1][0], before[1][1], f["pts"], R, t, VOXEL, 0, np.inf)["counts"], i
        else:
            skipped += 1
            assert kf.mapFrameOverlap() == (0, 0, 0), i
        for a, b in zip(columns(on), columns(off)):  # the option changes no bit of the map
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), i
    assert matched > 10000 and skipped < len(drive)
    assert np.array_equal(bits(np.asarray(on.trajectory())), bits(np.asarray(off.trajectory())))
    on.setMapOverlap(False)
    assert on.mapFrameOverlap() == (0, 0, 0)


@pytest.mark.parametrize("device_frontend", [True, False])
def test_query_by_hand_and_errors(natives, drive, device_frontend):
    p = pipeline(False, device_frontend)
    probe = drive[1]["pts"]
    with pytest.raises(RuntimeError):
        p.mapQuery(probe, np.eye(4))  # accumulation is off
    with pytest.raises(RuntimeError):
        p.mapOverlap(probe, np.eye(4))
    p.setMapAccumulation(VOXEL, evidence=EVIDENCE)
    counts, row, d2 = p.mapQuery(probe, np.eye(4))  # no frame folded yet: an empty map
    assert counts == counts_of(p, probe, np.eye(4), 1, np.inf) and counts[1:] == (0, 0) and np.all(row == -1) and np.all(np.isposinf(d2))
    assert p.mapOverlap(probe[:0], np.eye(4)) == (0, 0, 0)
    for i, f in enumerate(drive[:4]):
        feed(p, "cloud", i, f)
    T = np.asarray(p.currentPose())
    rows, keys, ev = columns(p)
    before = [c.tobytes() for c in (rows, keys, ev)]
    for cloud, pose in ((drive[3]["pts"], T), (drive[5]["pts"] * 1.05, T), (drive[0]["pts"][:333], np.eye(4))):
        for reach in (0, 1):
            want = Q.query(rows, keys, cloud, pose[:3, :3], np.array(pose[:3, 3]), VOXEL, reach, MAX_DIST, ev=ev)
            Q.same(p.mapQuery(cloud, pose, reach, MAX_DIST, with_keys=True, with_evidence=True), want, (reach, "all columns"))
            got = p.mapQuery(cloud, pose, reach, MAX_DIST)
            assert len(got) == 3 and got[0] == want["counts"] and got[1].tobytes() == want["row"].tobytes() and got[2].tobytes() == want["d2"].tobytes()
            assert p.mapOverlap(cloud, pose, reach, MAX_DIST) == want["counts"]
            assert want["counts"][1] > 100
    counts = p.mapOverlap(drive[3]["pts"], T, 0, 2 * VOXEL)  # the scan just folded, at its own pose: every candidate finds its own voxel
    assert counts[0] == counts[1] == counts[2] == drive[3]["pts"].shape[0]
    assert [c.tobytes() for c in columns(p)] == before  # the map is only read
    bad_T = T.copy()
    bad_T[1, 3] = np.nan
    for args in ((probe, bad_T), (probe, T, 2), (probe, T, -1), (probe, T, 1, -1.0), (probe, T, 1, np.nan), (probe[:, :2], T), (probe, T[:3])):
        with pytest.raises(ValueError):
            p.mapQuery(*args)
        with pytest.raises(ValueError):
            p.mapOverlap(*args)
    for args in ((True, 2), (True, 1, -0.5), (True, 1, np.nan)):
        with pytest.raises(ValueError):
            p.setMapOverlap(*args)
    with pytest.raises(RuntimeError):
        p.mapQuery(probe, T, with_attribute=True)  # the map has no attribute column
    plain = pipeline(False, device_frontend)
    plain.setMapAccumulation(VOXEL, with_attribute=True)
    feed(plain, "cloud", 0, drive[0])
    with pytest.raises(RuntimeError):
        plain.mapQuery(probe, T, with_evidence=True)  # ... and this one no evidence
    counts, row, d2, words = plain.mapQuery(drive[0]["pts"], np.asarray(plain.currentPose()), 0, np.inf, with_attribute=True)
    assert counts[0] == counts[1] == drive[0]["pts"].shape[0] and words.dtype == np.uint32 and not words.any()  # (frames without an attribute carry the word 0)
    assert [c.tobytes() for c in columns(p)] == before
