"""Pipeline.setMapAccumulation(moments=max_count) / mapMoments / mapSurfels on the 8-frame 16 x 450 synthetic drive of
tests/test_gpu_pipeline_registered_scan.py, both front-ends (the device map and the host twin): with moments=None poses, map, keys
and removal counts are those of a Pipeline that never heard of the keyword, bit for bit, and mapMoments is refused; with moments,
clearing and a range on, the map and its ten moment words are the restatement of tests/map_moments_ref.py (RefDrive: fold, clearing,
range prune) driven at the Pipeline's own poses, after every frame, and mapSurfels' centroids are the restatement's bits.
Everything is exact equality."""
import numpy as np
import pytest

import cloud_export_ref as E
import map_moments_ref as Mo
from test_gpu_pipeline_registered_scan import bits, drive, feed, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
RADIUS = 8.0  # the drive advances 1 m per frame: a prune every second frame
MARGIN = 0.25
ORIGIN = np.array([0.0, 0.0, 0.125])


@pytest.mark.parametrize("device_frontend", [True, False])
def test_moments_none_is_a_pipeline_that_never_heard_of_it(natives, drive, device_frontend):
    none, never = pipeline(False, device_frontend), pipeline(False, device_frontend)
    none.setMapAccumulation(VOXEL, moments=None)
    never.setMapAccumulation(VOXEL)
    for p in (none, never):
        p.setMapClearing(True, MARGIN, ORIGIN)
        p.setMapRange(RADIUS)
    assert not none.mapWithMoments()
    for i, f in enumerate(drive):
        feed(none, "cloud", i, f)
        feed(never, "cloud", i, f)
        assert np.array_equal(bits(np.asarray(none.currentPose())), bits(np.asarray(never.currentPose()))), i
        assert none.mapSize() == never.mapSize() and none.mapRemoved() == never.mapRemoved(), i
        assert E.same_bits(none.mapCloud(), never.mapCloud()) and none.mapKeys().tobytes() == never.mapKeys().tobytes(), i
    assert none.mapRemoved() > 0 and not np.array_equal(np.asarray(none.trajectory())[-1], np.eye(4))
    for call in (none.mapMoments, none.mapSurfels):
        with pytest.raises(RuntimeError):
            call()


@pytest.mark.parametrize("max_count,params", [(3, None), (1000, (2, 1, 6))])
@pytest.mark.parametrize("device_frontend", [True, False])
def test_drive_map_and_moments_after_every_frame(natives, drive, device_frontend, max_count, params):
    on, off = pipeline(False, device_frontend), pipeline(False, device_frontend)
    on.setMapAccumulation(VOXEL, with_attribute=True, evidence=params, moments=max_count)
    on.setMapClearing(True, MARGIN, ORIGIN)
    on.setMapRange(RADIUS)
    assert on.mapWithMoments() and on.mapMoments().shape == (0, 10) and on.mapSurfels()[0].shape == (0, 3)
    ref = Mo.RefDrive(VOXEL, max_count, params, RADIUS, margin=MARGIN, origin=ORIGIN)
    for i, f in enumerate(drive):
        feed(on, "cloud", i, f)
        feed(off, "cloud", i, f)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        T = np.asarray(on.currentPose())
        assert ref.frame(f["pts"], T) is not None
        assert on.mapSize() == ref.map.size and on.mapRemoved() == ref.removed and not on.mapOverflowed(), i
        assert E.same_bits(on.mapCloud(), ref.map.rows()) and on.mapKeys().tobytes() == ref.map.stored_keys().tobytes(), i
        mom, want = on.mapMoments(), ref.map.moments()
        assert mom.dtype == np.uint64 and mom.shape == want.shape and mom.tobytes() == want.tobytes(), i
        if params is not None:
            assert on.mapEvidence().tobytes() == ref.map.evidence().tobytes(), i
        c, nrm, eig, cnt = on.mapSurfels()
        assert c.dtype == np.float32 and E.same_bits(c, Mo.centroids(want, ref.map.stored_keys(), VOXEL)), i
        assert cnt.dtype == np.uint32 and cnt.tolist() == want[:, 0].tolist(), i
        assert nrm.shape == eig.shape == c.shape and np.all(np.isfinite(nrm)) and np.all(np.isfinite(eig)) and np.all(nrm[cnt < 3] == 0.0), i
        if i > 2:
            tail = on.mapMoments(first_row=mom.shape[0] - 3)
            assert tail.tobytes() == mom[-3:].tobytes()
            assert E.same_bits(on.mapSurfels(first_row=mom.shape[0] - 3)[0], c[-3:])
    assert ref.cleared > 0 and ref.removed > ref.cleared
    n = ref.map.moments()[:, 0]
    assert n.max() > 1 and (max_count != 3 or np.count_nonzero(n >= 3) > 0)  # voxels that took several points; some frozen
    on.clearMap()
    assert on.mapSize() == 0 and on.mapMoments().shape == (0, 10)


def test_errors(natives, drive):
    p = pipeline(False, True)
    for bad in (0, -1, 2 ** 31 + 1):
        with pytest.raises(ValueError):
            p.setMapAccumulation(VOXEL, moments=bad)
    with pytest.raises(RuntimeError):
        p.mapMoments()  # accumulation is off
    p.setMapAccumulation(VOXEL, moments=2 ** 31)
    feed(p, "cloud", 0, drive[0])
    with pytest.raises(ValueError):
        p.mapMoments(first_row=p.mapSize() + 1)
    with pytest.raises(ValueError):
        p.mapSurfels(first_row=p.mapSize() + 1)
    with pytest.raises(RuntimeError):
        p.mapEvidence()  # made without that column
    n = p.mapSize()
    assert n > 0 and int(p.mapMoments()[:, 0].sum()) > n
    p.setMapAccumulation(VOXEL, moments=2 ** 31)  # the same bound: the map stays
    assert p.mapSize() == n
    p.setMapAccumulation(VOXEL, moments=7)  # another: a new, empty map
    assert p.mapSize() == 0 and p.mapWithMoments()
