"""Pipeline.computeSourcesStamped — one frame from several sensors' byte records — against the paths it must equal bit for bit:
compute(stamp, cloud, stamps) fed the arrays the host twin (madicp_host_ingest_sources) prepared, with either front-end;
computeRecordsStamped on the unsplit records where the split reassembles exactly; compute where deskew = False ignores the time
fields.  The scan size and drive length of tests/test_gpu_pipeline_records_stamped.py."""
import numpy as np
import pytest

import ingest_records_ref as R
import ingest_sources_ref as SR
from fixtures import B_MAX, B_MIN
from mad_icp_amd import capi, synth
from mad_icp_amd.records import Source

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
    """base-frame scans quantised to 2^-8 (ingest_sources_ref.quantised) with about 2 % far records inserted, and uint32 times"""
    scene = synth.Scene(0)
    rng = np.random.default_rng(44)
    frames = []
    for i in range(N_FRAMES):
        sc = SR.quantised(synth.render_scan(scene, synth.path_pose(1.0 * i), 100 + i, n_beams=16, n_azimuth=450))
        n_bad = sc.shape[0] // 50
        xyz = np.insert(sc, rng.integers(0, sc.shape[0], size=n_bad), np.full((n_bad, 3), 400.0, np.float32), axis=0)
        frames.append((np.ascontiguousarray(xyz), rng.integers(SR.TIME_SHIFT, 10**8, size=xyz.shape[0]).astype("<u4")))
    return frames


def two_heads(xyz32, ticks, seed):
    """the frame as a rig delivers it: two heads with general extrinsics, each holding half of the base-frame points expressed in
    its own frame (rounded to float32 there), uint32 nanoseconds counted from each head's own message header"""
    h = xyz32.shape[0] // 2
    out = []
    for k, (sl, lay) in enumerate(((slice(0, h), SR.L22), (slice(h, None), SR.RecordLayout(48, 0, 4, 8, 21, R.T_U32)))):
        T = SR.rigid(seed + k)
        sensor = ((xyz32[sl].astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
        header = 250000 * k                                            # ns: the second head's message starts 0.25 ms later
        t = ticks[sl]
        local = np.where(t >= header, t - np.uint32(header), 0).astype("<u4")
        out.append(Source(R.pack(lay, sensor, local, seed=seed + k).reshape(-1).view(R.view_dtype(lay)), LO + 0.1 * k, HI - 10.0 * k,
                          sensor_to_base=T, time_scale=1e-9, time_offset=header * 1e-9))
    return out


@pytest.mark.parametrize("device_frontend", [True, False])
def test_equals_compute_with_the_host_twins_arrays(natives, drive, device_frontend):
    from mad_icp.src.pybind import pypeline as m

    A, B = m.Pipeline(*pipeline_args(True)), m.Pipeline(*pipeline_args(True))
    for p in (A, B):
        p.setDeviceFrontEnd(device_frontend)
    for i, (xyz32, ticks) in enumerate(drive):
        sources = two_heads(xyz32, ticks, 200 + 2 * i)
        pts, stamps, _, per = capi.host_ingest_sources(sources)
        assert min(per) > 1000 and sum(per) < xyz32.shape[0] and 0.0 <= stamps.min() < stamps.max() <= 1.0
        A.compute(0.1 * i, pts, stamps)
        B.computeSourcesStamped(0.1 * i, sources)
        assert np.array_equal(bits(np.asarray(A.currentPose())), bits(np.asarray(B.currentPose()))), i
        assert A.keyframeID() == B.keyframeID(), i
        assert A.isMapUpdated() == B.isMapUpdated(), i
    assert np.array_equal(bits(np.asarray(A.trajectory())), bits(np.asarray(B.trajectory())))
    assert not np.array_equal(np.asarray(A.trajectory())[-1], np.eye(4))


def test_exact_reassembly_is_compute_records_stamped(natives, drive):
    from mad_icp.src.pybind import pypeline as m

    A, B = m.Pipeline(*pipeline_args(True)), m.Pipeline(*pipeline_args(True))
    for i, (xyz32, ticks) in enumerate(drive):
        whole, sources = SR.reassembly(xyz32, ticks)
        A.computeRecordsStamped(0.1 * i, whole, LO, HI, layout=tuple(SR.L22))
        B.computeSourcesStamped(0.1 * i, sources)
        assert np.array_equal(bits(np.asarray(A.currentPose())), bits(np.asarray(B.currentPose()))), i
        assert A.keyframeID() == B.keyframeID() and A.isMapUpdated() == B.isMapUpdated(), i
    assert not np.array_equal(np.asarray(A.trajectory())[-1], np.eye(4))


def test_without_deskew_is_compute_and_bad_input_is_a_value_error(natives, drive):
    """deskew = False: the time fields and time_range are ignored; what the helper or the ingest refuses is a ValueError and
    leaves the Pipeline usable"""
    from mad_icp.src.pybind import pypeline as m

    A, B = m.Pipeline(*pipeline_args(False)), m.Pipeline(*pipeline_args(False))
    for i, (xyz32, ticks) in enumerate(drive[:5]):
        sources = two_heads(xyz32, ticks, 300 + 2 * i)
        pts, _, _, _ = capi.host_ingest_sources(sources)
        A.compute(0.1 * i, pts)
        for bad in ([], [sources[0]] * 9, [sources[0], Source(sources[1].records, LO, HI, time_scale=0.0)],
                    [sources[0], Source(sources[1].records, LO, HI, time_field=False)],
                    [Source(sources[0].records, LO, HI, sensor_to_base=np.full((4, 4), np.nan))]):
            with pytest.raises(ValueError):
                B.computeSourcesStamped(0.1 * i, bad)
        with pytest.raises(ValueError):
            B.computeSourcesStamped(0.1 * i, sources, time_range=(1.0, 1.0))
        B.computeSourcesStamped(0.1 * i, sources, time_range=(0.0, 0.05))
        assert np.array_equal(bits(np.asarray(A.currentPose())), bits(np.asarray(B.currentPose()))), i
        assert A.keyframeID() == B.keyframeID() and A.isMapUpdated() == B.isMapUpdated()
    assert A.currentID() == B.currentID()
