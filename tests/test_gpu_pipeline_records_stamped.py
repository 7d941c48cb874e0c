"""Pipeline.computeRecordsStamped — one frame straight from a driver's byte records with a time field — against the paths it
must equal bit for bit: compute(stamp, cloud, stamps) fed the arrays this TEST prepared on the host (tests/ingest_records_ref.py),
computeRecords where the time field does not matter, and itself across the two ways of handing the records over."""
import numpy as np
import pytest

import ingest_records_ref as R
import oracle_lib as O
from fixtures import B_MAX, B_MIN
from mad_icp_amd import records, synth

pytestmark = pytest.mark.gpu

HZ = 10.0
N_FRAMES = 8
LO, HI = 0.7, 120.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def pipeline_args(deskew):
    return (HZ, deskew, B_MAX, 0.1, 0.8, B_MIN, 0.02, 16, 8, False)


@pytest.fixture(scope="module")
def drive():
    """the drive of tests/test_gpu_deskew_stamped.py as float32, with about 5 % inserted records the filter drops (too near, too
    far, a NaN coordinate) so that it compacts, and random per-point times"""
    scene = synth.Scene(0)
    rng = np.random.default_rng(43)
    frames = []
    for i in range(N_FRAMES):
        sc = synth.render_scan(scene, synth.path_pose(1.0 * i), 100 + i, n_beams=16, n_azimuth=450).astype(np.float32)
        n_bad = sc.shape[0] // 20
        bad = rng.normal(size=(n_bad, 3)).astype(np.float32)
        bad /= np.linalg.norm(bad, axis=1, keepdims=True)
        kind = rng.integers(3, size=n_bad)
        bad = bad * np.where(kind == 0, 0.2, 400.0)[:, None].astype(np.float32)
        bad[kind == 2, rng.integers(3, size=int((kind == 2).sum()))] = np.nan
        xyz = np.insert(sc, rng.integers(0, sc.shape[0], size=n_bad), bad, axis=0)
        frames.append((np.ascontiguousarray(xyz), rng.uniform(0.0, 0.1, xyz.shape[0])))
    return frames


def times_for(lay, seconds):
    return (seconds * 1e9).astype("<u4") if lay.t_type == records.T_U32 else seconds.astype(R.TIME_DTYPE[lay.t_type])


@pytest.mark.parametrize("layout", ["xyzirt22", "ouster48"])
@pytest.mark.parametrize("device_frontend", [True, False])
def test_equals_compute_with_host_prepared_arrays(natives, drive, device_frontend, layout):
    from mad_icp.src.pybind import pypeline as m

    lay = R.LAYOUTS[layout]
    A, B = m.Pipeline(*pipeline_args(True)), m.Pipeline(*pipeline_args(True))
    for p in (A, B):
        p.setDeviceFrontEnd(device_frontend)
    for i, (xyz32, seconds) in enumerate(drive):
        buf = R.pack(lay, xyz32, times_for(lay, seconds), seed=i)
        pts, stamps_ref, _ = R.reference(buf, lay, LO, HI, 0)
        with np.errstate(invalid="ignore"):
            assert R.same_bits(pts, O.ingest_f32(xyz32, LO, HI, 0)) and pts.shape[0] < xyz32.shape[0]
        A.compute(0.1 * i, pts, stamps_ref)
        B.computeRecordsStamped(0.1 * i, buf.reshape(-1).view(R.view_dtype(lay)), LO, HI)
        assert np.array_equal(bits(np.asarray(A.currentPose())), bits(np.asarray(B.currentPose()))), i
        assert A.keyframeID() == B.keyframeID(), i
        assert A.isMapUpdated() == B.isMapUpdated(), i
    assert np.array_equal(bits(np.asarray(A.trajectory())), bits(np.asarray(B.trajectory())))
    assert not np.array_equal(np.asarray(A.trajectory())[-1], np.eye(4))


def _kitti_records(xyz32, seconds):
    rec = np.empty((xyz32.shape[0], 4), np.float32)
    rec[:, :3], rec[:, 3] = xyz32, seconds
    return rec


@pytest.mark.parametrize("kitti", [False, True])
def test_without_deskew_is_compute_records(natives, drive, kitti):
    """deskew = False: the time field (the 4th float of the KITTI layout) is ignored entirely"""
    from mad_icp.src.pybind import pypeline as m

    A, B = m.Pipeline(*pipeline_args(False)), m.Pipeline(*pipeline_args(False))
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<f4")])
    for i, (xyz32, seconds) in enumerate(drive[:5]):
        rec = _kitti_records(xyz32, seconds)
        A.computeRecords(0.1 * i, rec, LO, HI, kitti)
        B.computeRecordsStamped(0.1 * i, rec.reshape(-1).view(dt), LO, HI, kitti)
        assert np.array_equal(bits(np.asarray(A.currentPose())), bits(np.asarray(B.currentPose()))), i
        assert A.keyframeID() == B.keyframeID() and A.isMapUpdated() == B.isMapUpdated()


def test_without_a_time_field_is_compute_records_azimuth_deskew_included(natives, drive):
    from mad_icp.src.pybind import pypeline as m

    A, B, Cc = (m.Pipeline(*pipeline_args(True)) for _ in range(3))
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])
    dt_t = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<f4")])
    for i, (xyz32, seconds) in enumerate(drive[:5]):
        rec = _kitti_records(xyz32, seconds)
        A.computeRecords(0.1 * i, rec, LO, HI)
        B.computeRecordsStamped(0.1 * i, rec.reshape(-1).view(dt), LO, HI)                       # no time field in the dtype
        Cc.computeRecordsStamped(0.1 * i, rec.reshape(-1).view(dt_t), LO, HI, time_field=False)  # one that is ignored
        for p in (B, Cc):
            assert np.array_equal(bits(np.asarray(A.currentPose())), bits(np.asarray(p.currentPose()))), i
            assert A.keyframeID() == p.keyframeID() and A.isMapUpdated() == p.isMapUpdated()


def test_structured_array_and_raw_bytes_with_layout_agree_and_bad_input_is_a_value_error(natives, drive):
    from mad_icp.src.pybind import pypeline as m

    lay = R.LAYOUTS["xyzirt22"]
    S, U, T = (m.Pipeline(*pipeline_args(True)) for _ in range(3))
    bad_dtypes = [np.dtype([("x", ">f4"), ("y", "<f4"), ("z", "<f4")]),                            # big-endian
                  np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8")]),                            # float64 coordinates
                  np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<u8")]),              # unsupported time dtype
                  np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "u1", (245,))]),     # itemsize 257
                  np.dtype(dict(names=["x", "y", "z"], formats=["<f4"] * 3, offsets=[0, 2, 6], itemsize=10))]  # itemsize 10
    for i, (xyz32, seconds) in enumerate(drive[:5]):
        buf = R.pack(lay, xyz32, times_for(lay, seconds), seed=i)
        arr = buf.reshape(-1).view(R.view_dtype(lay))
        S.computeRecordsStamped(0.1 * i, arr, LO, HI)
        U.computeRecordsStamped(0.1 * i, buf, LO, HI, layout=tuple(lay))
        for dt in bad_dtypes:
            with pytest.raises(ValueError):
                T.computeRecordsStamped(0.1 * i, np.zeros(64, dt), LO, HI)
        with pytest.raises(ValueError):
            T.computeRecordsStamped(0.1 * i, buf, LO, HI)                                         # raw bytes without a layout
        with pytest.raises(ValueError):
            T.computeRecordsStamped(0.1 * i, arr[::2], LO, HI)                                    # not contiguous
        with pytest.raises(ValueError):
            T.computeRecordsStamped(0.1 * i, arr, LO, HI, time_field="stamp")                     # no such field
        with pytest.raises(ValueError):
            T.computeRecordsStamped(0.1 * i, arr, LO, HI, time_range=(1.0, 1.0))
        T.computeRecordsStamped(0.1 * i, arr, LO, HI, time_field="t")  # still usable, nothing of the refused calls stuck
        for p in (U, T):
            assert np.array_equal(bits(np.asarray(S.currentPose())), bits(np.asarray(p.currentPose()))), i
        assert T.currentID() == S.currentID()
