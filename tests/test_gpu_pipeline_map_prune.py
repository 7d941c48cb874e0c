"""Pipeline.setMapRange / mapPrune / mapRemoved / mapNewRows — a voxel map that follows the vehicle — on the 8-frame 16 x 450 drive
of tests/test_gpu_pipeline_registered_scan.py, both front-ends: the option changes no pose; after every frame the map is the
restatement of tests/map_prune_ref.py (RefDrive: the folds, the prune policy and the consumer's cursor) driven over the clouds the
frames' trees were built from at the frames' own poses, bit for bit; no row is delivered twice; a drive that overflows a small
max_points without a range does not with one.  Everything is exact equality."""
import numpy as np
import pytest

import cloud_export_ref as E
import map_prune_ref as P
from test_gpu_pipeline_attribute import feed as feed_indexed
from test_gpu_pipeline_attribute import with_index
from test_gpu_pipeline_map import built_from
from test_gpu_pipeline_registered_scan import bits, drive, feed, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
RADIUS = 8.0  # the drive advances 1 m per frame: a prune every second frame; below the sensor's range, so rows come and go


def row_set(rows):
    return set(map(bytes, np.ascontiguousarray(rows).view(np.uint8).reshape(rows.shape[0], 12)))


@pytest.mark.parametrize("kind,device_frontend", [("stamped", True), ("stamped", False), ("cloud", True), ("cloud", False)])
def test_drive_pose_bits_map_bits_and_the_stream(natives, drive, kind, device_frontend):
    deskew = kind == "stamped"
    on, plain, off = pipeline(deskew, device_frontend), pipeline(deskew, device_frontend), pipeline(deskew, device_frontend)
    on.setMapAccumulation(VOXEL)
    on.setMapRange(RADIUS)
    plain.setMapAccumulation(VOXEL)  # accumulation without a range
    assert on.mapRange() == RADIUS and plain.mapRange() == 0.0 and off.mapRange() == 0.0 and on.mapRemoved() == 0
    assert on.mapNewRows().shape == (0, 3)
    ref = P.RefDrive(VOXEL, RADIUS)
    stream, want_stream, since_prune = [], [], set()
    for i, f in enumerate(drive):
        for p in (on, plain, off):
            feed(p, kind, i, f)
        for other in (plain, off):
            assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(other.currentPose()))), i
            assert on.keyframeID() == other.keyframeID() and on.isMapUpdated() == other.isMapUpdated(), i
        T = np.asarray(on.currentPose())
        cloud = built_from("stamped", f, i, np.asarray(on.trajectory())) if deskew else f["pts"]
        prunes = ref.prunes
        assert ref.frame(cloud, T) is not None
        assert on.mapSize() == ref.map.size and on.mapRemoved() == ref.removed and not on.mapOverflowed(), i
        assert E.same_bits(on.mapCloud(), ref.map.rows()), i
        if i % 3 != 1:  # (the consumer does not look after every frame)
            got, (want, _) = on.mapNewRows(), ref.new_rows()
            assert got.dtype == np.float32 and E.same_bits(got, want), i
            assert on.mapNewRows().shape == (0, 3)
            if ref.prunes != prunes:
                since_prune = set()
            new = row_set(got)
            assert len(new) == got.shape[0] and not (new & since_prune), i  # no duplicate between two prunes
            since_prune |= new
            stream.append(got)
            want_stream.append(want)
    assert ref.prunes >= 3 and ref.removed > 5000 and plain.mapSize() > on.mapSize() and plain.mapRemoved() == 0
    assert np.concatenate(stream).tobytes() == np.concatenate(want_stream).tobytes()
    assert np.array_equal(bits(np.asarray(on.trajectory())), bits(np.asarray(off.trajectory())))
    assert not np.array_equal(np.asarray(on.trajectory())[-1], np.eye(4))


@pytest.mark.parametrize("device_frontend", [True, False])
def test_small_max_points_overflows_without_a_range_only(natives, drive, device_frontend):
    # the first two frames fit (about 2 100 + 800 rows, 7 179 points each), the third does not: 2 932 + 7 179 > 9 700
    max_points = 9700
    on, without = pipeline(False, device_frontend), pipeline(False, device_frontend)
    on.setMapAccumulation(VOXEL, max_points=max_points)
    on.setMapRange(RADIUS)
    without.setMapAccumulation(VOXEL, max_points=max_points)
    ref, ref_without = P.RefDrive(VOXEL, RADIUS, max_points), P.RefDrive(VOXEL, 0.0, max_points)
    by_capacity = 0
    for i, f in enumerate(drive):
        feed(on, "cloud", i, f)
        feed(without, "cloud", i, f)
        T = np.asarray(on.currentPose())
        assert np.array_equal(bits(T), bits(np.asarray(without.currentPose()))), i
        refused = ref.map.size + f["pts"].shape[0] > max_points
        prunes = ref.prunes
        assert ref.frame(f["pts"], T) is not None and not ref.overflowed  # the restatement stays under max_points
        by_capacity += int(refused and ref.prunes > prunes)
        ref_without.frame(f["pts"], T)
        assert not on.mapOverflowed() and on.mapSize() == ref.map.size <= max_points and E.same_bits(on.mapCloud(), ref.map.rows()), i
        assert without.mapOverflowed() == ref_without.overflowed and without.mapSize() == ref_without.map.size, i
    assert by_capacity >= 1 and ref.prunes > by_capacity  # both rules pruned: before a fold that would not fit, and by distance
    assert without.mapOverflowed() and E.same_bits(without.mapCloud(), ref_without.map.rows())  # existing behaviour


@pytest.mark.parametrize("device_frontend", [True, False])
def test_prune_by_hand_clear_and_errors(natives, drive, device_frontend):
    p = pipeline(False, device_frontend)
    for bad in (-1.0, float("nan"), float("inf"), 1e200):
        with pytest.raises(ValueError):
            p.setMapRange(bad)
    p.setMapRange(RADIUS)  # no effect while accumulation is off
    for call in (lambda: p.mapPrune(np.zeros(3), 1.0), p.mapNewRows):
        with pytest.raises(RuntimeError):
            call()
    p.setMapRange(0.0)
    p.setMapAccumulation(VOXEL)
    assert p.mapPrune(np.zeros(3), 1.0) == 0  # no frame folded yet
    ref = P.RefDrive(VOXEL)
    for i, f in enumerate(drive[:3]):
        feed(p, "cloud", i, f)
        T = np.asarray(p.currentPose())
        ref.frame(f["pts"], T)
    first, (want, _) = p.mapNewRows(), ref.new_rows()
    assert E.same_bits(first, want) and first.shape[0] == p.mapSize() > 1000 and p.mapRemoved() == 0
    for bad_c, bad_r in ((np.array([0.0, np.nan, 0.0]), 5.0), (np.zeros(3), 0.0), (np.zeros(3), -1.0), (np.zeros(3), float("inf")),
                         (np.zeros(3), 1e200), (np.zeros(2), 5.0)):
        with pytest.raises(ValueError):
            p.mapPrune(bad_c, bad_r)
    assert E.same_bits(p.mapCloud(), ref.map.rows())
    c = T[:3, 3] + np.array([0.3125, 0.0, -0.5])
    removed = p.mapPrune(c, 6.0)
    assert removed == ref.prune(c, 6.0) > 0 and p.mapRemoved() == removed and p.mapSize() == ref.map.size > 0
    assert E.same_bits(p.mapCloud(), ref.map.rows()) and p.mapNewRows().shape == (0, 3)  # everything kept had been fetched
    feed(p, "cloud", 3, drive[3])
    T = np.asarray(p.currentPose())
    added = ref.frame(drive[3]["pts"], T)
    got, (want, _) = p.mapNewRows(), ref.new_rows()
    assert got.shape[0] == added > 0 and E.same_bits(got, want) and not (row_set(got) & row_set(p.mapCloud()[:p.mapSize() - added]))
    # clearMap: the cursor and the count start again
    p.clearMap()
    ref.clear()
    assert p.mapSize() == 0 and p.mapRemoved() == 0 and p.mapNewRows().shape == (0, 3)
    feed(p, "cloud", 4, drive[4])
    T = np.asarray(p.currentPose())
    ref.frame(drive[4]["pts"], T)
    got = p.mapNewRows()
    assert got.shape[0] == p.mapSize() > 0 and E.same_bits(got, ref.new_rows()[0]) and E.same_bits(got, p.mapCloud())
    with pytest.raises(RuntimeError):
        p.mapNewRows(with_attribute=True)  # the map was made without the column


@pytest.mark.parametrize("device_frontend", [True, False])
def test_new_rows_with_the_record_index(natives, drive, device_frontend):
    """the attribute is the record index: row j of what mapNewRows delivers after a frame is the deskew of that frame's record
    attr[j], taken through the frame's pose — whatever was pruned in between"""
    p = pipeline(True, device_frontend)
    p.setMapAccumulation(VOXEL, with_attribute=True)
    p.setMapRange(RADIUS)
    ref = P.RefDrive(VOXEL, RADIUS)
    delivered = 0
    for i, f in enumerate(drive):
        rec, kept, sources, _ = with_index(f)
        feed_indexed(p, "records", i, rec, sources)
        T = np.asarray(p.currentPose())
        cloud = built_from("records", f, i, np.asarray(p.trajectory()))
        assert ref.frame(cloud, T, kept) is not None
        rows, attr = p.mapNewRows(with_attribute=True)
        want_rows, want_attr = ref.new_rows()
        assert E.same_bits(rows, want_rows) and attr.dtype == np.dtype("<u4") and np.array_equal(attr, want_attr), i
        survivor = np.searchsorted(kept, attr)  # record index -> the survivor's place in the cloud
        assert np.array_equal(kept[survivor], attr)
        assert E.same_bits(rows, E.export_f32(cloud[survivor], T[:3, :3], T[:3, 3], 0.0)), i
        full_rows, full_attr = p.mapCloud(0, with_attribute=True)
        assert E.same_bits(full_rows, ref.map.rows()) and np.array_equal(full_attr, ref.map.attr()), i
        delivered += rows.shape[0]
    assert ref.prunes >= 3 and delivered > p.mapSize() > 0
