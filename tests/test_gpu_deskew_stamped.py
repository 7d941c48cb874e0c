"""Motion compensation from per-point timestamps on the device: fe::deskew_stamped through madicp_cloud_deskew_stamped, and
Pipeline.compute(stamp, cloud, timestamps) on top of it.

The kernel is held to three things at once: the chunk rule of tests/deskew_stamped_ref.py exactly, the host twin
(madicp_host_deskew_stamped) bit for bit — which is what makes the Pipeline equivalence at the end exact — and the numpy
restatement within 1e-12 m (|p| <= 120 m: three products and three additions of magnitudes up to 120 m, each within 2^-53
relative, are ~1e-13 m; the pose tables come from the same libm)."""
import ctypes as C

import numpy as np
import pytest

import deskew_stamped_ref as R
from fixtures import B_MAX, B_MIN
from mad_icp_amd import capi, synth

pytestmark = pytest.mark.gpu

HZ = R.HZ
POS_TOL = 1e-12


def cloud(n, seed, r_max=120.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, r_max, (n, 1)))


def host(pts, stamps, vel):
    Tp, Tn = R.poses_for(vel, HZ)
    return capi.host_deskew_stamped(pts, stamps, Tp, Tn, HZ)  # (cloud, the six doubles of the velocity, chunks)


def device(ctx, pts, stamps, v6):
    cid = ctx.cloud_upload(pts)
    try:
        chunks = ctx.cloud_deskew_stamped(cid, stamps, v6, HZ, want_chunks=True)
        return ctx.cloud_download(cid), chunks
    finally:
        ctx.cloud_release(cid)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# one point past ONE trip of the launch geometry — min((n + 255) / 256, 8 * CUs) workgroups of 256 threads, 256 CUs on an MI355X:
# the grid-stride loop takes its second trip (on a part with fewer CUs it takes more of them)
SECOND_TRIP = 256 * 8 * 256 + 1


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]


def check_size(ctx, n):
    pts, s = cloud(n, 100 + n % 1000), R.mixed_stamps(n, seed=1)
    want_chunks = R.chunk_of(s)
    for vname, vel in R.VELOCITIES.items():
        h_out, v6, h_chunks = host(pts, s, vel)
        d_out, d_chunks = device(ctx, pts, s, v6)
        assert np.array_equal(d_chunks, want_chunks), vname
        assert np.array_equal(h_chunks, want_chunks), vname
        assert np.array_equal(bits(d_out), bits(h_out)), vname        # bit-equal to the host twin
        err = np.abs(d_out - R.compensate(pts, s, v6, HZ)).max()       # row i of the output is point i: input order
        assert err <= POS_TOL, (vname, err)
        if vname == "zero":
            assert np.array_equal(d_out, pts)


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_rule_host_twin_and_numpy(ctx, n):
    check_size(ctx, n)


def test_kernel_second_trip_of_the_stride_loop(ctx):
    check_size(ctx, SECOND_TRIP)


@pytest.mark.parametrize("name", ["uniform", "centres", "boundaries", "specials"])
def test_kernel_stamp_families(ctx, name):
    s = R.SPECIALS.copy() if name == "specials" else R.family(name)  # (the specials in the order listed)
    pts = cloud(s.size, 7)
    h_out, v6, _ = host(pts, s, R.VELOCITIES["crossing"])
    d_out, d_chunks = device(ctx, pts, s, v6)
    assert np.array_equal(d_chunks, R.chunk_of(s))
    if name == "specials":
        assert d_chunks.tolist() == R.SPECIAL_CHUNKS.tolist()
    assert np.array_equal(bits(d_out), bits(h_out))


def test_physical_sign_convention(ctx):
    vel = R.PHYSICAL_VEL
    p, s, w, bound = R.physical_scan(4000, vel, HZ, r_max=60.0)
    _, v6, _ = host(p, s, vel)
    out, _ = device(ctx, p, s, v6)
    err = np.linalg.norm(out - w, axis=1).max()
    print("physical: max error %.4e m, bound %.4e m, ratio %.3f" % (err, bound, err / bound))
    assert err <= bound


def test_scratch_and_buffers(ctx):
    """small, larger (the scratch grows), small again; a stamped and an azimuth deskew back to back; a deskewed cloud built into
    a tree that equals the tree of the host twin's output byte for byte"""
    vel = R.VELOCITIES["rodrigues"]
    for n in (500, 30000, 500):
        pts, s = cloud(n, n + 11), R.mixed_stamps(n, seed=n)
        h_out, v6, h_chunks = host(pts, s, vel)
        d_out, d_chunks = device(ctx, pts, s, v6)
        assert np.array_equal(d_chunks, h_chunks) and np.array_equal(bits(d_out), bits(h_out))
    # back to back on one context: the two deskews share the pose table's place in the scratch
    n = 5000
    pts, s = cloud(n, 21, r_max=60.0), R.mixed_stamps(n, seed=21)
    h_out, v6, _ = host(pts, s, vel)
    ca, cb, cc = ctx.cloud_upload(pts), ctx.cloud_upload(pts), ctx.cloud_upload(pts)
    ctx.cloud_deskew_stamped(ca, s, v6, HZ)
    ctx.cloud_deskew(cb, v6, HZ)
    ctx.cloud_deskew_stamped(cc, s, v6, HZ)
    az_first = ctx.cloud_download(cb)
    assert np.array_equal(bits(ctx.cloud_download(ca)), bits(h_out))
    assert np.array_equal(bits(ctx.cloud_download(cc)), bits(h_out))
    ctx.cloud_release(cb)
    cb = ctx.cloud_upload(pts)
    ctx.cloud_deskew(cb, v6, HZ)  # (the azimuth path after a stamped one: the same cloud as before it)
    assert np.array_equal(bits(ctx.cloud_download(cb)), bits(az_first))
    # deskewed, then built
    t_dev, nl_dev = ctx.tree_build(ca, B_MAX, B_MIN)
    ch = ctx.cloud_upload(h_out)
    t_ref, nl_ref = ctx.tree_build(ch, B_MAX, B_MIN)
    assert nl_dev == nl_ref
    assert ctx.tree_download(t_dev, 2 * nl_dev - 1).tobytes() == ctx.tree_download(t_ref, 2 * nl_ref - 1).tobytes()
    for t in (t_dev, t_ref):
        ctx.tree_release(t)
    for c in (ca, cb, cc, ch):
        ctx.cloud_release(c)


def test_rejections_leave_the_cloud(ctx):
    """host-side refusals: nothing is launched, the cloud still downloads to its original bytes"""
    L = capi.hip_lib()
    dp = C.POINTER(C.c_double)
    n = 300
    pts, s = cloud(n, 31), R.mixed_stamps(n, seed=31)
    v6 = np.ascontiguousarray(R.VELOCITIES["rodrigues"])
    S, V = s.ctypes.data_as(dp), v6.ctypes.data_as(dp)
    cid = ctx.cloud_upload(pts)
    INVALID, CAPACITY = -1, -4
    assert L.madicp_cloud_deskew_stamped(ctx._h, cid, S, n - 1, V, HZ, None) == INVALID       # n mismatch
    assert L.madicp_cloud_deskew_stamped(ctx._h, cid, S, n + 1, V, HZ, None) == INVALID
    assert L.madicp_cloud_deskew_stamped(ctx._h, cid, None, n, V, HZ, None) == INVALID        # null stamps
    assert L.madicp_cloud_deskew_stamped(ctx._h, cid, S, n, None, HZ, None) == INVALID        # null velocity
    assert L.madicp_cloud_deskew_stamped(None, cid, S, n, V, HZ, None) == INVALID             # null context
    assert L.madicp_cloud_deskew_stamped(ctx._h, 987654, S, n, V, HZ, None) == INVALID        # unknown id
    assert L.madicp_cloud_deskew_stamped(ctx._h, cid, S, n, V, 0.0, None) == INVALID          # sensor_hz = 0
    assert L.madicp_cloud_deskew_stamped(ctx._h, cid, S, n, V, -10.0, None) == INVALID
    with pytest.raises(capi.MadIcpError, match="sensor_hz"):
        ctx.cloud_deskew_stamped(cid, s, v6, 0.0)
    with pytest.raises(capi.MadIcpError, match="n mismatch"):
        ctx.cloud_deskew_stamped(cid, s[:-1], v6, HZ)
    assert np.array_equal(bits(ctx.cloud_download(cid)), bits(pts))
    # a look-ahead build in flight owns the builder's scratch
    ctx.tree_build_begin(cloud(2000, 32, r_max=40.0), B_MAX, B_MIN)
    try:
        assert L.madicp_cloud_deskew_stamped(ctx._h, cid, S, n, V, HZ, None) == CAPACITY
        with pytest.raises(capi.MadIcpError, match="look-ahead tree build is in flight"):
            ctx.cloud_deskew_stamped(cid, s, v6, HZ)
    finally:
        ctx.tree_build_cancel()
    assert np.array_equal(bits(ctx.cloud_download(cid)), bits(pts))
    # ... and the cloud is as usable as before
    chunks = ctx.cloud_deskew_stamped(cid, s, v6, HZ, want_chunks=True)
    assert np.array_equal(chunks, R.chunk_of(s))
    ctx.cloud_release(cid)


# ---- Pipeline --------------------------------------------------------------------------------------------------------------------
N_FRAMES = 8


@pytest.fixture(scope="module")
def drive():
    scene = synth.Scene(0)
    scans = [synth.render_scan(scene, synth.path_pose(1.0 * i), 100 + i, n_beams=16, n_azimuth=450) for i in range(N_FRAMES)]
    rng = np.random.default_rng(41)
    stamps = [rng.uniform(0.0, 1.0, sc.shape[0]) for sc in scans]
    return scans, stamps


def pipeline_args(deskew):
    return (HZ, deskew, B_MAX, 0.1, 0.8, B_MIN, 0.02, 16, 8, False)


@pytest.mark.parametrize("device_frontend", [True, False])
def test_pipeline_equals_the_precompensated_drive(natives, drive, device_frontend):
    """B: deskew = True, fed compute(stamp, cloud, stamps).  A: deskew = False, fed the cloud this TEST compensated with the host
    twin from A's own last two poses (the raw cloud before frame 2).  Same bits at every frame: the device kernel is bit-equal
    to the host twin (above), and `deskew` touches nothing else in the frame step."""
    from mad_icp.src.pybind import pypeline as m

    scans, stamps = drive
    A, B = m.Pipeline(*pipeline_args(False)), m.Pipeline(*pipeline_args(True))
    for p in (A, B):
        p.setDeviceFrontEnd(device_frontend)
    for i, (sc, st) in enumerate(zip(scans, stamps)):
        fed = sc
        if i >= 2:
            traj = np.asarray(A.trajectory())
            fed, _, _ = capi.host_deskew_stamped(sc, st, traj[-2], traj[-1], HZ)
            assert not np.array_equal(fed, sc)
        A.compute(0.1 * i, fed)
        B.compute(0.1 * i, sc, st)
        assert np.array_equal(bits(np.asarray(A.currentPose())), bits(np.asarray(B.currentPose()))), i
        assert A.keyframeID() == B.keyframeID(), i
        assert A.isMapUpdated() == B.isMapUpdated(), i
    assert np.array_equal(bits(np.asarray(A.trajectory())), bits(np.asarray(B.trajectory())))


@pytest.mark.parametrize("device_frontend", [True, False])
def test_pipeline_without_deskew_ignores_the_stamps(natives, drive, device_frontend):
    from mad_icp.src.pybind import pypeline as m

    scans, stamps = drive
    two, three, vec = (m.Pipeline(*pipeline_args(False)) for _ in range(3))
    for p in (two, three, vec):
        p.setDeviceFrontEnd(device_frontend)
    for i, (sc, st) in enumerate(zip(scans[:5], stamps[:5])):
        two.compute(0.1 * i, sc)
        three.compute(0.1 * i, sc, st)
        vec.compute(0.1 * i, m.VectorEigen3d(sc), st.astype(np.float32))  # (the container overload; float32 stamps are cast)
        for p in (three, vec):
            assert np.array_equal(bits(np.asarray(two.currentPose())), bits(np.asarray(p.currentPose()))), i
            assert two.keyframeID() == p.keyframeID() and two.isMapUpdated() == p.isMapUpdated()


def test_pipeline_wrong_length_is_a_value_error(natives, drive):
    from mad_icp.src.pybind import pypeline as m

    scans, stamps = drive
    good, tried = m.Pipeline(*pipeline_args(True)), m.Pipeline(*pipeline_args(True))
    for i, (sc, st) in enumerate(zip(scans[:5], stamps[:5])):
        good.compute(0.1 * i, sc, st)
        with pytest.raises(ValueError):
            tried.compute(0.1 * i, sc, st[:-1])
        with pytest.raises(ValueError):
            tried.compute(0.1 * i, m.VectorEigen3d(sc), np.concatenate([st, [0.5]]))
        with pytest.raises(ValueError):
            tried.compute(0.1 * i, sc, st.reshape(-1, 1))
        tried.compute(0.1 * i, sc, st)  # still usable, and nothing of the refused calls stuck
        assert np.array_equal(bits(np.asarray(good.currentPose())), bits(np.asarray(tried.currentPose()))), i
        assert tried.currentID() == good.currentID()
