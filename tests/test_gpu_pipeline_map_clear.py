"""Pipeline.setMapClearing / mapClearRays — free-space clearing of the voxel map by every folded scan — on the 8-frame 16 x 450 drive
of tests/test_gpu_pipeline_registered_scan.py, both front-ends: the option changes no pose on the arrays, the records and the
sources feed; after every frame the map is the restatement of tests/map_clear_ref.py (RefDrive: fold, clearing, range prune, the
consumer's cursor) driven over the clouds the frames' trees were built from at the frames' own poses, bit for bit; no row is
delivered twice across clearings and prunes together; clearMap starts the cursor again.  Everything is exact equality."""
import numpy as np
import pytest

import cloud_export_ref as E
import map_clear_ref as Cl
from test_gpu_pipeline_map import built_from
from test_gpu_pipeline_registered_scan import bits, drive, feed, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
RADIUS = 8.0  # the drive advances 1 m per frame: a prune every second frame
MARGIN = 0.25
ORIGIN = np.array([0.0, 0.0, 0.125])


def row_set(rows):
    return set(map(bytes, np.ascontiguousarray(rows).view(np.uint8).reshape(rows.shape[0], 12)))


@pytest.mark.parametrize("kind,device_frontend", [("stamped", True), ("stamped", False), ("cloud", True), ("cloud", False),
                                                  ("records", True), ("sources", True)])
def test_drive_pose_bits_map_bits_and_the_stream(natives, drive, kind, device_frontend):
    deskew = kind != "cloud"
    on, plain, off = pipeline(deskew, device_frontend), pipeline(deskew, device_frontend), pipeline(deskew, device_frontend)
    on.setMapAccumulation(VOXEL)
    on.setMapClearing(True, MARGIN, ORIGIN)
    on.setMapRange(RADIUS)
    plain.setMapAccumulation(VOXEL)  # accumulation alone
    off.setMapClearing(True)  # no effect while accumulation is off
    assert on.mapClearing() and not plain.mapClearing() and on.mapRemoved() == 0 and on.mapNewRows().shape == (0, 3)
    ref = Cl.RefDrive(VOXEL, RADIUS, margin=MARGIN, origin=ORIGIN)
    stream, want_stream = [], []
    for i, f in enumerate(drive):
        for p in (on, plain, off):
            feed(p, kind, i, f)
        for other in (plain, off):
            assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(other.currentPose()))), i
            assert on.keyframeID() == other.keyframeID() and on.isMapUpdated() == other.isMapUpdated(), i
        T = np.asarray(on.currentPose())
        cloud = built_from(kind, f, i, np.asarray(on.trajectory())) if deskew else f["pts"]
        assert ref.frame(cloud, T) is not None
        assert on.mapSize() == ref.map.size and on.mapRemoved() == ref.removed and not on.mapOverflowed(), i
        assert E.same_bits(on.mapCloud(), ref.map.rows()), i
        if i % 3 != 1:  # (the consumer does not look after every frame)
            got, (want, _) = on.mapNewRows(), ref.new_rows()
            assert got.dtype == np.float32 and E.same_bits(got, want), i
            assert on.mapNewRows().shape == (0, 3)
            stream.append(got)
            want_stream.append(want)
    # both kinds of removal happened, and the map is smaller for it
    assert ref.cleared > 500 and ref.removed > ref.cleared and ref.prunes >= 3 and plain.mapSize() > on.mapSize() and plain.mapRemoved() == 0
    assert np.concatenate(stream).tobytes() == np.concatenate(want_stream).tobytes()
    # at most once: the vehicle moves, so a voxel that was cleared and filled again holds another float — every delivered row is distinct
    everything = np.concatenate(stream)
    assert len(row_set(everything)) == everything.shape[0] > on.mapSize()
    assert np.array_equal(bits(np.asarray(on.trajectory())), bits(np.asarray(off.trajectory())))
    assert not np.array_equal(np.asarray(on.trajectory())[-1], np.eye(4))


@pytest.mark.parametrize("device_frontend", [True, False])
def test_clearing_by_hand_clear_and_errors(natives, drive, device_frontend):
    p = pipeline(False, device_frontend)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            p.setMapClearing(True, bad)
    for bad in (np.array([0.0, np.nan, 0.0]), np.array([np.inf, 0.0, 0.0]), np.zeros(2)):
        with pytest.raises(ValueError):
            p.setMapClearing(True, 0.0, bad)
    assert not p.mapClearing()
    with pytest.raises(RuntimeError):
        p.mapClearRays(drive[0]["pts"], np.eye(4))  # accumulation is off
    p.setMapAccumulation(VOXEL)
    assert p.mapClearRays(drive[0]["pts"], np.eye(4)) == 0  # no frame folded yet
    ref = Cl.RefDrive(VOXEL, clearing=False)
    for i, f in enumerate(drive[:3]):
        feed(p, "cloud", i, f)
        T = np.asarray(p.currentPose())
        ref.frame(f["pts"], T)
    first, (want, _) = p.mapNewRows(), ref.new_rows()
    assert E.same_bits(first, want) and first.shape[0] == p.mapSize() > 1000 and p.mapRemoved() == 0
    cloud = drive[2]["pts"] * 1.5  # the last scan, half as far again: looks through much of what it folded
    bad_T = T.copy()
    bad_T[1, 3] = np.nan
    for args in ((cloud, bad_T), (cloud, T, np.array([0.0, np.inf, 0.0])), (cloud, T, np.zeros(3), -1.0), (cloud, T, np.zeros(3), np.nan),
                 (cloud[:, :2], T), (cloud, T[:3]), (cloud, T, np.zeros(4))):
        with pytest.raises(ValueError):
            p.mapClearRays(*args)
    assert E.same_bits(p.mapCloud(), ref.map.rows()) and p.mapRemoved() == 0
    removed = p.mapClearRays(cloud, T, ORIGIN, MARGIN)
    assert removed == ref.clear_rays(cloud, T, ORIGIN, MARGIN) > 100 and p.mapRemoved() == removed and p.mapSize() == ref.map.size > 0
    assert E.same_bits(p.mapCloud(), ref.map.rows()) and p.mapNewRows().shape == (0, 3)  # everything kept had been fetched
    pruned = p.mapPrune(T[:3, 3], 9.0)
    assert pruned == ref.prune(T[:3, 3], 9.0) > 0 and p.mapRemoved() == removed + pruned == ref.removed  # both kinds counted
    feed(p, "cloud", 3, drive[3])
    T = np.asarray(p.currentPose())
    added = ref.frame(drive[3]["pts"], T)
    got, (want, _) = p.mapNewRows(), ref.new_rows()
    assert got.shape[0] == added > 0 and E.same_bits(got, want) and E.same_bits(p.mapCloud(), ref.map.rows())
    # clearMap: the cursor and the count start again; the option, switched on now, acts from the next fold
    p.clearMap()
    ref.clear()
    p.setMapClearing(True, MARGIN, ORIGIN)
    ref.clearing, ref.margin, ref.origin = True, MARGIN, ORIGIN
    assert p.mapSize() == 0 and p.mapRemoved() == 0 and p.mapNewRows().shape == (0, 3)
    for i in (4, 5):
        feed(p, "cloud", i, drive[i])
        ref.frame(drive[i]["pts"], np.asarray(p.currentPose()))
    got = p.mapNewRows()
    assert got.shape[0] == p.mapSize() > 0 and E.same_bits(got, ref.new_rows()[0]) and E.same_bits(got, p.mapCloud())
    assert p.mapRemoved() == ref.removed > 0
    p.setMapClearing(False)
    feed(p, "cloud", 6, drive[6])
    ref.clearing = False
    ref.frame(drive[6]["pts"], np.asarray(p.currentPose()))
    assert p.mapRemoved() == ref.removed and E.same_bits(p.mapCloud(), ref.map.rows())


@pytest.mark.parametrize("first_frontend", [True, False])
def test_the_front_end_switched_mid_drive(natives, drive, first_frontend):
    """the map lives where its first fold put it; after setDeviceFrontEnd the scans cross over for their fold and their clearing"""
    p = pipeline(False, first_frontend)
    p.setMapAccumulation(VOXEL, with_attribute=True)
    p.setMapClearing(True, MARGIN, ORIGIN)
    ref = Cl.RefDrive(VOXEL, margin=MARGIN, origin=ORIGIN)
    for i, f in enumerate(drive[:6]):
        if i == 3:
            p.setDeviceFrontEnd(not first_frontend)
        feed(p, "cloud", i, f)
        ref.frame(f["pts"], np.asarray(p.currentPose()))
        assert p.mapRemoved() == ref.removed and E.same_bits(p.mapCloud(), ref.map.rows()), i
    assert ref.removed > 0
