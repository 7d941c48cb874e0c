"""CPU suite: the host twin of the stamped deskew (madicp_host_deskew_stamped, csrc/host/deskew.cpp: deskew_cloud_stamped) against
the plain restatement of tests/deskew_stamped_ref.py — the chunk of every stamp exactly, positions within 1e-12 m, the physical
sign convention, the two branches of the chunk poses, bad arguments."""
import ctypes as C

import numpy as np
import pytest

import deskew_stamped_ref as R

HZ = R.HZ
# |p| <= 120 m: three products and three additions of magnitudes up to 120 m, each within 2^-53 relative, are ~1e-13 m; the pose
# tables come from the same libm
POS_TOL = 1e-12


@pytest.fixture(scope="module")
def capi(natives):
    from mad_icp_amd import capi as c

    return c


def cloud(n, seed, r_max=120.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, r_max, (n, 1)))


def run(capi, pts, stamps, vel, hz=HZ):
    Tp, Tn = R.poses_for(vel, hz)
    out, v, chunks = capi.host_deskew_stamped(pts, stamps, Tp, Tn, hz)
    assert np.abs(v - vel).max() <= 1e-9 * max(1.0, np.abs(vel).max())  # (the log map gives the velocity back)
    return out, v, chunks


def test_restatement_boundaries_and_specials():
    """properties of the rule itself, in numpy: every boundary value lands in the upper bin (its lower neighbour may round up to
    it as well: s * 1023 + 0.5 is rounded twice — which is why the device and the host must evaluate it the same way)"""
    b = R.boundaries()
    k = np.arange(1023)
    assert np.array_equal(R.chunk_of(b[:, 1]), k + 1)
    lower = R.chunk_of(b[:, 0])
    assert ((lower == k) | (lower == k + 1)).all() and (lower == k).any()
    assert np.array_equal(R.chunk_of(b[:, 2]), k + 1)
    assert np.array_equal(R.chunk_of(R.centres()), np.arange(1024))
    assert np.array_equal(R.chunk_of(R.SPECIALS), R.SPECIAL_CHUNKS)


@pytest.mark.parametrize("name", ["uniform", "centres", "boundaries", "specials"])
def test_chunks_equal_the_rule(capi, name):
    s = R.family(name)
    pts = cloud(s.size, 1)
    _, _, chunks = run(capi, pts, s, R.VELOCITIES["rodrigues"])
    assert np.array_equal(chunks, R.chunk_of(s))


def test_specials_in_order(capi):
    _, _, chunks = run(capi, cloud(R.SPECIALS.size, 2), R.SPECIALS, R.VELOCITIES["crossing"])
    assert chunks.tolist() == R.SPECIAL_CHUNKS.tolist()


@pytest.mark.parametrize("vname", list(R.VELOCITIES))
def test_positions_and_velocity_branches(capi, vname):
    vel = R.VELOCITIES[vname]
    fo = R.first_order_chunks(vel, HZ)
    if vname in ("zero", "first_order"):
        assert fo.all()
    elif vname == "rodrigues":
        assert not fo[:1022].any()
    else:  # the table crosses theta^2 = 1e-8 near chunk 921
        first = int(np.argmax(fo))
        assert 915 <= first <= 927 and not fo[:first].any() and fo[first:].all()
    n = 6000
    pts, s = cloud(n, 3), R.mixed_stamps(n, seed=3)
    out, v, chunks = run(capi, pts, s, vel)
    assert np.array_equal(chunks, R.chunk_of(s))
    ref = R.compensate(pts, s, v, HZ)  # (with the velocity the host derived: the same six doubles)
    err = np.abs(out - ref).max()
    print("max |host - numpy| = %.3e m" % err)
    assert err <= POS_TOL
    if vname == "zero":
        assert np.array_equal(out, pts)


def test_large_cloud_takes_the_task_pool(capi):
    """(past 16 384 points the host splits the cloud into pieces for the task pool: same result)"""
    n = 40001
    pts, s = cloud(n, 4), R.mixed_stamps(n, seed=4)
    out, v, chunks = run(capi, pts, s, R.VELOCITIES["rodrigues"])
    assert np.array_equal(chunks, R.chunk_of(s))
    assert np.abs(out - R.compensate(pts, s, v, HZ)).max() <= POS_TOL


def test_physical_sign_convention(capi):
    """a sensor moving with the naive model; compensation with the true velocity returns the world points within half a chunk of
    motion — a flipped sign or a reversed time axis misses by metres"""
    vel = R.PHYSICAL_VEL
    p, s, w, bound = R.physical_scan(4000, vel, HZ, r_max=60.0)
    out, _, _ = run(capi, p, s, vel)
    err = np.linalg.norm(out - w, axis=1).max()
    print("physical: max error %.4e m, bound %.4e m, ratio %.3f" % (err, bound, err / bound))
    assert err <= bound
    # the wrong conventions, for scale
    wrong, _, _ = run(capi, p, 1.0 - s, vel)
    assert np.linalg.norm(wrong - w, axis=1).max() > 100 * bound


def test_bad_arguments_leave_the_buffer(capi):
    L = capi.host_lib()
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pts = cloud(50, 5)
    keep = pts.copy()
    s = R.mixed_stamps(50)
    T = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
    T2 = capi.pose12(R.poses_for(R.VELOCITIES["rodrigues"], HZ)[1])
    P, S, A, B = (a.ctypes.data_as(dp) for a in (pts, s, T, T2))
    assert L.madicp_host_deskew_stamped(None, S, 50, A, B, HZ, None, None) < 0
    assert L.madicp_host_deskew_stamped(P, None, 50, A, B, HZ, None, None) < 0
    assert L.madicp_host_deskew_stamped(P, S, -1, A, B, HZ, None, None) < 0
    assert L.madicp_host_deskew_stamped(P, S, 50, None, B, HZ, None, None) < 0
    assert L.madicp_host_deskew_stamped(P, S, 50, A, None, HZ, None, None) < 0
    for hz in (0.0, -10.0, float("nan")):
        assert L.madicp_host_deskew_stamped(P, S, 50, A, B, hz, None, None) < 0
    assert np.array_equal(pts, keep)
    # and the good call, without the optional outputs
    assert L.madicp_host_deskew_stamped(P, S, 50, A, B, HZ, None, None) == 0
    assert not np.array_equal(pts, keep)
    assert L.madicp_host_deskew_stamped(P, S, 0, A, B, HZ, None, None) == 0
