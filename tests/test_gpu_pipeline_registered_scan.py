"""Pipeline.setKeepScan / registeredScan — the registered scan out — on the 8-frame 16 x 450 drive of
tests/test_gpu_pipeline_records_stamped.py: the option changes no pose; the exported scan is the numpy restatement of
tests/cloud_export_ref.py applied to the cloud the frame's tree was built from (the input, or madicp_host_deskew_stamped of it
with the two previous poses) at the frame's own pose; every feed of the same frame exports the same bytes; the errors."""
import numpy as np
import pytest

import cloud_export_ref as E
import ingest_records_ref as R
import ingest_sources_ref as SR
from fixtures import B_MAX, B_MIN
from mad_icp_amd import capi, synth
from mad_icp_amd.records import Source

pytestmark = pytest.mark.gpu

HZ = 10.0
N_FRAMES = 8
LO, HI = 0.7, 120.0
LAY = SR.L22  # packed XYZIRT with uint32 nanoseconds


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def pipeline(deskew, device_frontend=True, keep=False):
    from mad_icp.src.pybind import pypeline as m

    p = m.Pipeline(HZ, deskew, B_MAX, 0.1, 0.8, B_MIN, 0.02, 16, 8, False)
    p.setDeviceFrontEnd(device_frontend)
    if keep:
        p.setKeepScan(True)
    return p


def two_heads(xyz32, ticks, seed):
    """the frame as a two-head rig delivers it (tests/test_gpu_pipeline_sources_stamped.py)"""
    h = xyz32.shape[0] // 2
    out = []
    for k, (sl, lay) in enumerate(((slice(0, h), SR.L22), (slice(h, None), SR.RecordLayout(48, 0, 4, 8, 21, R.T_U32)))):
        T = SR.rigid(seed + k)
        sensor = ((xyz32[sl].astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
        header = 250000 * k
        t = ticks[sl]
        local = np.where(t >= header, t - np.uint32(header), 0).astype("<u4")
        out.append(Source(R.pack(lay, sensor, local, seed=seed + k), LO + 0.1 * k, HI - 10.0 * k, layout=lay, sensor_to_base=T,
                          time_scale=1e-9, time_offset=header * 1e-9))
    return out


@pytest.fixture(scope="module")
def drive():
    """per frame: the byte records of one head and of a two-head rig, and the arrays the host prepares from each (points, stamps)"""
    scene = synth.Scene(0)
    rng = np.random.default_rng(43)
    frames = []
    for i in range(N_FRAMES):
        sc = SR.quantised(synth.render_scan(scene, synth.path_pose(1.0 * i), 100 + i, n_beams=16, n_azimuth=450))
        n_bad = sc.shape[0] // 50
        xyz32 = np.ascontiguousarray(np.insert(sc, rng.integers(0, sc.shape[0], size=n_bad), np.full((n_bad, 3), 400.0, np.float32), axis=0))
        ticks = rng.integers(SR.TIME_SHIFT, 10**8, size=xyz32.shape[0]).astype("<u4")
        buf = R.pack(LAY, xyz32, ticks, seed=i)
        pts, stamps, _ = R.reference(buf, LAY, LO, HI, 0)
        sources = two_heads(xyz32, ticks, 200 + 2 * i)
        s_pts, s_stamps, _, _ = SR.reference(sources)
        frames.append(dict(records=buf.reshape(-1).view(R.view_dtype(LAY)), pts=pts, stamps=stamps, sources=sources, s_pts=s_pts,
                           s_stamps=s_stamps))
    assert frames[0]["pts"].shape[0] > 5000
    return frames


def feed(p, kind, i, f):
    if kind == "cloud":
        p.compute(0.1 * i, f["pts"])
    elif kind == "stamped":
        p.compute(0.1 * i, f["pts"], f["stamps"])
    elif kind == "records":
        p.computeRecordsStamped(0.1 * i, f["records"], LO, HI)
    elif kind == "sources":
        p.computeSourcesStamped(0.1 * i, f["sources"])
    elif kind == "sources_as_arrays":
        p.compute(0.1 * i, f["s_pts"], f["s_stamps"])
    else:
        raise AssertionError(kind)


@pytest.mark.parametrize("kind,device_frontend", [("cloud", True), ("cloud", False), ("stamped", True), ("stamped", False),
                                                  ("records", True), ("sources", True)])
def test_the_option_changes_no_pose(natives, drive, kind, device_frontend):
    on, off = pipeline(True, device_frontend, keep=True), pipeline(True, device_frontend)
    assert on.keepScan() and not off.keepScan()
    for i, f in enumerate(drive):
        feed(on, kind, i, f)
        feed(off, kind, i, f)
        assert np.array_equal(bits(np.asarray(on.currentPose())), bits(np.asarray(off.currentPose()))), i
        assert on.keyframeID() == off.keyframeID() and on.isMapUpdated() == off.isMapUpdated(), i
        assert on.registeredScanSize() == (f["s_pts"] if kind == "sources" else f["pts"]).shape[0]
    assert np.array_equal(bits(np.asarray(on.trajectory())), bits(np.asarray(off.trajectory())))
    assert not np.array_equal(np.asarray(on.trajectory())[-1], np.eye(4))


@pytest.mark.parametrize("device_frontend", [True, False])
def test_without_deskew_the_scan_is_the_input(natives, drive, device_frontend):
    p = pipeline(False, device_frontend, keep=True)
    for i, f in enumerate(drive[:5]):
        p.compute(0.1 * i, f["pts"])
        got = p.registeredScan(0.0, "sensor")
        assert got.dtype == np.float32 and np.array_equal(got, f["pts"].astype(np.float32))
        T = np.asarray(p.currentPose())
        for v in (0.0, 0.3):
            assert E.same_bits(p.registeredScan(v, "map"), E.export_f32(f["pts"], T[:3, :3], T[:3, 3], v)), (i, v)
        assert E.same_bits(p.registeredScan(voxel_size=0.3, frame="sensor"), E.export_f32(f["pts"], np.eye(3), np.zeros(3), 0.3))
        assert E.same_bits(p.registeredScan(), E.export_f32(f["pts"], T[:3, :3], T[:3, 3], 0.0))  # defaults: every point, map frame


@pytest.mark.parametrize("device_frontend", [True, False])
def test_with_deskew_the_scan_is_the_compensated_cloud(natives, drive, device_frontend):
    """stamped frames: from frame 2 on the tree is built from madicp_host_deskew_stamped of the input with the two previous poses
    (bit-equal on both front-ends for the same poses); each front-end is held to ITS OWN trajectory"""
    p = pipeline(True, device_frontend, keep=True)
    for i, f in enumerate(drive):
        p.compute(0.1 * i, f["pts"], f["stamps"])
        traj = np.asarray(p.trajectory())
        assert traj.shape[0] == i + 1
        cloud = f["pts"]
        if i >= 2:
            cloud, _, _ = capi.host_deskew_stamped(f["pts"], f["stamps"], traj[i - 2], traj[i - 1], HZ)
            assert not np.array_equal(cloud, f["pts"])
        T = np.asarray(p.currentPose())
        assert E.same_bits(p.registeredScan(0.0, "sensor"), E.export_f32(cloud, np.eye(3), np.zeros(3), 0.0)), i
        for v in (0.0, 0.3):
            got = p.registeredScan(v, "map")
            assert E.same_bits(got, E.export_f32(cloud, T[:3, :3], T[:3, 3], v)), (i, v)
        assert 100 < got.shape[0] < cloud.shape[0]


@pytest.mark.parametrize("kind,as_arrays", [("records", "stamped"), ("sources", "sources_as_arrays")])
def test_feeds_agree(natives, drive, kind, as_arrays):
    """records and sources frames export the bytes of compute(stamp, cloud, stamps) fed the host-prepared arrays"""
    A, B = pipeline(True, True, keep=True), pipeline(True, True, keep=True)
    for i, f in enumerate(drive):
        feed(A, as_arrays, i, f)
        feed(B, kind, i, f)
        assert A.registeredScanSize() == B.registeredScanSize()
        for v, frame in ((0.0, "map"), (0.3, "map"), (0.0, "sensor")):
            a, b = A.registeredScan(v, frame), B.registeredScan(v, frame)
            assert a.shape[0] > 100 and a.tobytes() == b.tobytes(), (i, v, frame)


def test_azimuth_deskew_keeps_every_point_and_is_repeatable(natives, drive):
    """content is not pinned here: the device atan2 may differ from libm's in the last bit (include/madicp_hip.h)"""
    A, B = pipeline(True, True, keep=True), pipeline(True, True, keep=True)
    for i, f in enumerate(drive[:5]):
        A.compute(0.1 * i, f["pts"])
        B.compute(0.1 * i, f["pts"])
        assert A.registeredScanSize() == f["pts"].shape[0]
        a = A.registeredScan(0.0, "map")
        assert a.shape == (f["pts"].shape[0], 3)
        assert a.tobytes() == B.registeredScan(0.0, "map").tobytes()
        assert A.registeredScan(0.3, "map").tobytes() == B.registeredScan(0.3, "map").tobytes()


@pytest.mark.parametrize("device_frontend", [True, False])
def test_errors_and_lifetime(natives, drive, device_frontend):
    p = pipeline(False, device_frontend)
    with pytest.raises(RuntimeError):
        p.registeredScan()  # the option is off
    p.compute(0.0, drive[0]["pts"])
    with pytest.raises(RuntimeError):
        p.registeredScan()
    p.setKeepScan(True)
    assert p.registeredScanSize() == 0
    with pytest.raises(RuntimeError):
        p.registeredScan()  # on, but no frame has been computed since
    p.prefetch(drive[1]["pts"])  # stays legal: the frame builds synchronously
    p.compute(0.1, drive[1]["pts"])
    first = p.registeredScan(0.0, "sensor")
    assert np.array_equal(first, drive[1]["pts"].astype(np.float32))
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            p.registeredScan(bad, "map")
    with pytest.raises(ValueError):
        p.registeredScan(0.0, "world")
    # the scan of frame i is gone once compute of frame i + 1 has replaced it
    p.compute(0.2, drive[2]["pts"])
    second = p.registeredScan(0.0, "sensor")
    assert p.registeredScanSize() == drive[2]["pts"].shape[0] and np.array_equal(second, drive[2]["pts"].astype(np.float32))
    assert second.shape != first.shape or not np.array_equal(second, first)
    p.setKeepScan(False)
    assert not p.keepScan() and p.registeredScanSize() == 0
    with pytest.raises(RuntimeError):
        p.registeredScan()
    p.compute(0.3, drive[3]["pts"])  # and the Pipeline goes on
    with pytest.raises(RuntimeError):
        p.registeredScan()
