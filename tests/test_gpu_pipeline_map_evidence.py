"""Pipeline.setMapAccumulation(evidence=(hit, miss, cap)) / mapEvidence / mapConfirmed on the 8-frame 16 x 450 synthetic drive of
tests/test_gpu_pipeline_registered_scan.py, both front-ends (the device map and the host twin): with evidence=None poses and map
are those of a Pipeline that never heard of the keyword, bit for bit, and mapEvidence is refused; with evidence, clearing and a
range on, map and column are the restatement of tests/map_evidence_ref.py (RefDrive: fold, clearing, range prune) driven at the
Pipeline's own poses, after every frame; mapConfirmed is numpy filtering of mapCloud by mapEvidence.  Everything is exact equality."""
import numpy as np
import pytest

import cloud_export_ref as E
import map_clear_ref as Cl
import map_evidence_ref as Ev
from test_gpu_pipeline_registered_scan import bits, drive, feed, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
RADIUS = 8.0  # the drive advances 1 m per frame: a prune every second frame
MARGIN = 0.25
ORIGIN = np.array([0.0, 0.0, 0.125])


@pytest.mark.parametrize("device_frontend", [True, False])
def test_evidence_none_is_a_pipeline_that_never_heard_of_it(natives, drive, device_frontend):
    none, never = pipeline(False, device_frontend), pipeline(False, device_frontend)
    none.setMapAccumulation(VOXEL, evidence=None)
    never.setMapAccumulation(VOXEL)
    for p in (none, never):
        p.setMapClearing(True, MARGIN, ORIGIN)
        p.setMapRange(RADIUS)
    assert not none.mapWithEvidence()
    for i, f in enumerate(drive):
        feed(none, "cloud", i, f)
        feed(never, "cloud", i, f)
        assert np.array_equal(bits(np.asarray(none.currentPose())), bits(np.asarray(never.currentPose()))), i
        assert none.mapSize() == never.mapSize() and none.mapRemoved() == never.mapRemoved(), i
        assert E.same_bits(none.mapCloud(), never.mapCloud()) and none.mapKeys().tobytes() == never.mapKeys().tobytes(), i
    assert none.mapRemoved() > 0 and not np.array_equal(np.asarray(none.trajectory())[-1], np.eye(4))
    for call in (none.mapEvidence, lambda: none.mapConfirmed(1)):
        with pytest.raises(RuntimeError):
            call()


@pytest.mark.parametrize("params", [(1, 1, 1), (2, 1, 6)])
@pytest.mark.parametrize("device_frontend", [True, False])
def test_drive_map_and_column_after_every_frame(natives, drive, device_frontend, params):
    on, off = pipeline(False, device_frontend), pipeline(False, device_frontend)
    on.setMapAccumulation(VOXEL, with_attribute=True, evidence=params)
    on.setMapClearing(True, MARGIN, ORIGIN)
    on.setMapRange(RADIUS)
    assert on.mapWithEvidence() and on.mapEvidence().shape == (0,) and on.mapConfirmed(1).shape == (0, 3)
    ref = Ev.RefDrive(VOXEL, params, RADIUS, margin=MARGIN, origin=ORIGIN)
    plain = Cl.RefDrive(VOXEL, RADIUS, margin=MARGIN, origin=ORIGIN)
    for i, f in enumerate(drive):
        feed(on, "cloud", i, f)
        feed(off, "cloud", i, f)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        T = np.asarray(on.currentPose())
        assert ref.frame(f["pts"], T) is not None
        plain.frame(f["pts"], T)
        assert on.mapSize() == ref.map.size and on.mapRemoved() == ref.removed and not on.mapOverflowed(), i
        rows, ev = on.mapCloud(), on.mapEvidence()
        assert E.same_bits(rows, ref.map.rows()) and ev.dtype == np.uint32 and ev.tobytes() == ref.map.evidence().tobytes(), i
        assert on.mapKeys().tobytes() == ref.map.stored_keys().tobytes(), i
        if i > 2:
            tail = on.mapEvidence(first_row=ev.shape[0] - 3)
            assert tail.tobytes() == ev[-3:].tobytes()
        for min_e in (0, 1, 2, params[2], params[2] + 1):
            m = ev >= min_e
            got = on.mapConfirmed(min_e)
            assert got.dtype == np.float32 and got.shape == rows[m].shape and E.same_bits(got, np.ascontiguousarray(rows[m])), (i, min_e)
        r2, k2, w2 = on.mapConfirmed(2, with_keys=True, with_attribute=True)
        m = ev >= 2
        assert E.same_bits(r2, np.ascontiguousarray(rows[m])) and k2.tobytes() == on.mapKeys()[m].tobytes(), i
        assert np.asarray(w2).view(np.uint32).tobytes() == np.asarray(on.mapCloud(with_attribute=True)[1]).view(np.uint32)[m].tobytes(), i
        if params == (1, 1, 1):  # the plain map, row for row
            assert E.same_bits(rows, plain.map.rows()) and np.all(ev == 1), i
    assert ref.cleared > 0 and ref.removed > ref.cleared
    if params != (1, 1, 1):  # evidence keeps rows that one see-through would have removed, and has used some up all the same
        assert on.mapSize() > plain.map.size and len(set(on.mapEvidence().tolist())) > 2
    on.clearMap()
    assert on.mapSize() == 0 and on.mapEvidence().shape == (0,) and on.mapConfirmed(0).shape == (0, 3)


def test_errors(natives, drive):
    p = pipeline(False, True)
    for bad in ((0, 1, 1), (1, 0, 1), (2, 1, 1), (1, 1, 2 ** 31), (1, 1), (1, 1, -1)):
        with pytest.raises(ValueError):
            p.setMapAccumulation(VOXEL, evidence=bad)
    with pytest.raises(RuntimeError):
        p.mapEvidence()  # accumulation is off
    p.setMapAccumulation(VOXEL, evidence=(1, 1, 4))
    feed(p, "cloud", 0, drive[0])
    with pytest.raises(ValueError):
        p.mapEvidence(first_row=p.mapSize() + 1)
    with pytest.raises(RuntimeError):
        p.mapConfirmed(1, with_attribute=True)  # made without that column
    n = p.mapSize()
    assert n > 0 and np.all(p.mapEvidence() == 1)
    p.setMapAccumulation(VOXEL, evidence=(1, 1, 4))  # the same triple: the map stays
    assert p.mapSize() == n
    p.setMapAccumulation(VOXEL, evidence=(1, 2, 4))  # another: a new, empty map
    assert p.mapSize() == 0 and p.mapWithEvidence()
