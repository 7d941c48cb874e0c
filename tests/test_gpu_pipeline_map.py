"""Pipeline.setMapAccumulation / mapCloud — registered scans accumulated into a voxel map — on the 8-frame 16 x 450 drive of
tests/test_gpu_pipeline_registered_scan.py: the option changes no pose; after every frame the map is the numpy restatement of
tests/voxel_map_ref.py folded over the clouds the frames' trees were built from (the input, or madicp_host_deskew_stamped of it
with the two previous poses) at the frames' own poses, bit for bit; windows, keyframes only, overflow, the errors."""
import numpy as np
import pytest

import cloud_export_ref as E
import voxel_map_ref as V
from mad_icp_amd import capi
from test_gpu_pipeline_registered_scan import HZ, bits, drive, feed, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5


def built_from(kind, f, i, traj):
    """the cloud frame i's tree was built from, for a Pipeline with deskew = true fed stamps (from frame 2 on: compensated with the
    two previous poses) — obtained as tests/test_gpu_pipeline_registered_scan.py obtains it"""
    pts, stamps = (f["s_pts"], f["s_stamps"]) if kind == "sources" else (f["pts"], f["stamps"])
    if i < 2:
        return pts
    cloud, _, _ = capi.host_deskew_stamped(pts, stamps, traj[i - 2], traj[i - 1], HZ)
    assert not np.array_equal(cloud, pts)
    return cloud


def distinct_voxels(cloud, T, voxel):
    return E.export_f32(cloud, T[:3, :3], T[:3, 3], voxel).shape[0]


def check_not_vacuous(added, n_points, own):
    """every frame adds rows; from the second frame on fewer than it has points — most fall into voxels the map already has —
    and the map is smaller than the frames' own distinct-voxel counts together"""
    assert all(a > 0 for a in added), added
    assert all(a < n for a, n in zip(added[1:], n_points[1:])), (added, n_points)
    assert sum(added) < sum(own), (added, own)
    assert all(a < o for a, o in zip(added[1:], own[1:])), (added, own)


@pytest.mark.parametrize("kind,device_frontend", [("stamped", True), ("stamped", False), ("records", True), ("sources", True)])
def test_stamped_feeds_pose_bits_and_map_bits(natives, drive, kind, device_frontend):
    on, off = pipeline(True, device_frontend), pipeline(True, device_frontend)
    on.setMapAccumulation(VOXEL)
    assert on.mapVoxelSize() == VOXEL and off.mapVoxelSize() == 0.0 and on.mapSize() == 0
    ref = V.RefMap(VOXEL)
    added, n_points, own = [], [], []
    for i, f in enumerate(drive):
        feed(on, kind, i, f)
        feed(off, kind, i, f)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        assert on.keyframeID() == off.keyframeID() and on.isMapUpdated() == off.isMapUpdated(), i
        traj = np.asarray(on.trajectory())
        cloud, T = built_from(kind, f, i, traj), np.asarray(on.currentPose())
        before = ref.size
        added.append(ref.insert(cloud, T[:3, :3], T[:3, 3]))
        n_points.append(cloud.shape[0])
        own.append(distinct_voxels(cloud, T, VOXEL))
        assert on.mapSize() == ref.size, i
        got = on.mapCloud()
        assert got.dtype == np.float32 and got.shape == (ref.size, 3) and E.same_bits(got, ref.rows()), i
        assert on.mapCloud(before).tobytes() == got[before:].tobytes() and on.mapCloud(first_row=ref.size).shape == (0, 3)
        assert not on.mapOverflowed() and on.registeredScanSize() == 0  # (independent of setKeepScan: nothing is retained)
    assert np.array_equal(bits(np.asarray(on.trajectory())), bits(np.asarray(off.trajectory())))
    assert not np.array_equal(np.asarray(on.trajectory())[-1], np.eye(4))
    check_not_vacuous(added, n_points, own)


@pytest.mark.parametrize("device_frontend", [True, False])
def test_without_deskew_the_input_is_folded(natives, drive, device_frontend):
    """compute(stamp, cloud) with deskew = false: the tree is built from the input; with setKeepScan on beside it"""
    on, off = pipeline(False, device_frontend, keep=True), pipeline(False, device_frontend)
    on.setMapAccumulation(VOXEL)
    ref = V.RefMap(VOXEL)
    added, own = [], []
    for i, f in enumerate(drive):
        on.prefetch(f["pts"])  # stays legal: the frame builds synchronously
        feed(on, "cloud", i, f)
        feed(off, "cloud", i, f)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        T = np.asarray(on.currentPose())
        added.append(ref.insert(f["pts"], T[:3, :3], T[:3, 3]))
        own.append(distinct_voxels(f["pts"], T, VOXEL))
        assert on.mapSize() == ref.size and E.same_bits(on.mapCloud(), ref.rows()), i
        assert on.registeredScanSize() == f["pts"].shape[0]  # the retained scan is still there for registeredScan
        assert E.same_bits(on.registeredScan(VOXEL, "map"), E.export_f32(f["pts"], T[:3, :3], T[:3, 3], VOXEL))
    assert np.array_equal(bits(np.asarray(on.trajectory())), bits(np.asarray(off.trajectory())))
    check_not_vacuous(added, [f["pts"].shape[0] for f in drive], own)


def test_azimuth_deskew_changes_no_pose_and_is_repeatable(natives, drive):
    """compute(stamp, cloud) with deskew = true: the compensated cloud's content is not pinned (the device atan2 may differ from
    libm's in the last bit), the poses and the repeatability are"""
    A, B, off = pipeline(True, True), pipeline(True, True), pipeline(True, True)
    A.setMapAccumulation(VOXEL)
    B.setMapAccumulation(VOXEL)
    sizes = [0]
    for i, f in enumerate(drive[:5]):
        for p in (A, B, off):
            feed(p, "cloud", i, f)
        assert np.array_equal(bits(np.asarray(A.currentPose())), bits(np.asarray(off.currentPose()))), i
        assert A.mapCloud().tobytes() == B.mapCloud().tobytes()
        sizes.append(A.mapSize())
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[-1] < sum(f["pts"].shape[0] for f in drive[:5])


def test_keyframes_only(natives, drive):
    on, off = pipeline(True, True), pipeline(True, True)
    on.setMapAccumulation(VOXEL, keyframes_only=True)
    ref = V.RefMap(VOXEL)
    folded = []
    for i, f in enumerate(drive):
        feed(on, "stamped", i, f)
        feed(off, "stamped", i, f)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        if on.isMapUpdated():
            T = np.asarray(on.currentPose())
            ref.insert(built_from("stamped", f, i, np.asarray(on.trajectory())), T[:3, :3], T[:3, 3])
            folded.append(i)
        assert on.mapSize() == ref.size and E.same_bits(on.mapCloud(), ref.rows()), i
    assert folded and folded[0] == 0, folded  # the first frame is a keyframe


@pytest.mark.parametrize("device_frontend", [True, False])
def test_off_on_off_overflow_and_errors(natives, drive, device_frontend):
    p, off = pipeline(False, device_frontend), pipeline(False, device_frontend)
    for call in (p.mapSize, p.mapCloud, p.clearMap):
        with pytest.raises(RuntimeError):
            call()  # the option is off
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            p.setMapAccumulation(bad)
    with pytest.raises(ValueError):
        p.setMapAccumulation(VOXEL, max_points=0)
    n0, n1 = drive[0]["pts"].shape[0], drive[1]["pts"].shape[0]
    # max_points = the first frame's points: it fits exactly; the second is refused (the rows frame 0 left — a third of its points
    # at this voxel size — plus its own points exceed it), the poses go on unchanged, accumulation stops
    assert n1 > n0 // 2
    p.setMapAccumulation(VOXEL, max_points=n0)
    sizes = []
    for i, f in enumerate(drive[:4]):
        feed(p, "cloud", i, f)
        feed(off, "cloud", i, f)
        assert np.array_equal(bits(np.asarray(p.currentPose())), bits(np.asarray(off.currentPose()))), i
        assert p.mapOverflowed() == (i >= 1), i
        sizes.append(p.mapSize())
    assert sizes[0] + n1 > n0 and 0 < sizes[0] == sizes[1] == sizes[2] == sizes[3] < n0
    first = p.mapCloud()
    with pytest.raises(ValueError):
        p.mapCloud(sizes[0] + 1)
    # clearMap: the overflow is forgotten and accumulation resumes from an empty map
    p.clearMap()
    assert not p.mapOverflowed() and p.mapSize() == 0
    feed(p, "cloud", 4, drive[4])
    feed(off, "cloud", 4, drive[4])
    T = np.asarray(p.currentPose())
    assert np.array_equal(bits(T), bits(np.asarray(off.currentPose())))
    ref = V.RefMap(VOXEL)
    ref.insert(drive[4]["pts"], T[:3, :3], T[:3, 3])
    assert E.same_bits(p.mapCloud(), ref.rows()) and not p.mapOverflowed()
    # off frees the map; on again starts an empty one
    p.setMapAccumulation(0.0)
    assert p.mapVoxelSize() == 0.0 and not p.mapOverflowed()
    with pytest.raises(RuntimeError):
        p.mapCloud()
    feed(p, "cloud", 5, drive[5])
    feed(off, "cloud", 5, drive[5])
    p.setMapAccumulation(VOXEL)
    assert p.mapSize() == 0 and p.mapCloud().shape == (0, 3)
    feed(p, "cloud", 6, drive[6])
    feed(off, "cloud", 6, drive[6])
    T = np.asarray(p.currentPose())
    assert np.array_equal(bits(T), bits(np.asarray(off.currentPose())))
    ref = V.RefMap(VOXEL)
    ref.insert(drive[6]["pts"], T[:3, :3], T[:3, 3])
    assert E.same_bits(p.mapCloud(), ref.rows()) and first.shape[0] > 0


@pytest.mark.parametrize("first_frontend", [True, False])
def test_the_front_end_switched_mid_drive(natives, drive, first_frontend):
    """the map lives where its first fold put it — on the device or in the host twin; after setDeviceFrontEnd the scans come from
    the other side and cross over for their fold: the same rule, the same bytes"""
    p = pipeline(False, first_frontend)
    p.setMapAccumulation(VOXEL)
    ref = V.RefMap(VOXEL)
    for i, f in enumerate(drive[:6]):
        if i == 3:
            p.setDeviceFrontEnd(not first_frontend)
        feed(p, "cloud", i, f)
        T = np.asarray(p.currentPose())
        assert ref.insert(f["pts"], T[:3, :3], T[:3, 3]) > 0
        assert p.mapSize() == ref.size and E.same_bits(p.mapCloud(), ref.rows()), i
