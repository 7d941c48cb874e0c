"""Context.map_register_cloud (madicp_map_register_cloud: fe::map_surfels, fe::map_align_terms, fe::map_align_join,
fe::map_align_step) against the numpy restatement (tests/map_align_ref.py) fed THE DEVICE'S OWN map_download_surfels, and against
the host twin.  Linearise-only at every size around a wavefront, a workgroup and the tree's second and third level: counts, row and
e exactly equal, H, b, chi2 equal by value, the same call twice the same bits.  The traced five-round run: every row's sums are the
restatement's linearisation AT THE DEVICE'S X_k, exactly; every X_{k+1} lies within tests/test_gpu_gn_step.py's step tolerance of
the restatement's step from the device's H_k, b_k; round 0 moves the pose and reduces chi2.  Against the twin the final pose agrees
to 1e-5 m / 1e-5 rad and the counts are equal.  Maps with attribute and evidence columns, a map after a growth, a prune and a
clearing, the empty map, that the map is only read, every refusal."""
import ctypes as C

import numpy as np
import pytest

import gn_step_ref as G
import map_align_ref as A
from mad_icp_amd import capi
from map_impls import DevImpl
from test_host_map_align import CAPACITY, INVALID, MAX_COUNT, make_map, same_linearisation

pytestmark = pytest.mark.gpu

EYE = (np.eye(3), np.zeros(3))


def dev_map(ctx, folds=(), with_attr=False, evidence=None, initial_rows=64):
    """a device moments map with the folds in it; the caller closes it"""
    m = DevImpl(ctx, A.VOXEL, initial_rows, 1 << 22, with_attr, evidence, MAX_COUNT)
    for pts in folds:
        m.insert(pts, *EYE)
    return m


def columns(m):
    return m.rows(), m.keys(), m.surfels()


def everything(m):
    out = [m.rows(), m.keys(), m.moments(), *m.surfels()] + [c for c in (m.words(), m.evidence()) if c is not None]
    return [c.tobytes() for c in out]


@pytest.fixture(scope="module")
def corner(ctx):
    m = dev_map(ctx, A.map_folds())
    yield m, columns(m)
    m.close()


@pytest.fixture(scope="module")
def twin():
    h = make_map(A.map_folds())
    yield h
    capi.host_map_destroy(h)


@pytest.mark.parametrize("n", A.SIZES)
def test_linearise_only_is_the_restatement(corner, n):
    m, (rows, keys, surfels) = corner
    R, t = A.start_pose()
    cloud = A.scan(n)
    before = everything(m)
    for params in (A.DEFAULT, A.GATED, dict(A.GATED, reach=0)):
        want = A.linearize(rows, keys, surfels, cloud, R, t, **params)
        got = m.register(cloud, R, t, 0, per_point=True, **params)
        same_linearisation(got, want)
        assert np.array_equal(got["R"], R) and np.array_equal(got["t"], t) and np.array_equal(got["X"][0], np.concatenate([R.reshape(-1), t]))
        again = m.register(cloud, R, t, 0, per_point=True, **params)
        for key in ("R", "t", "X", "H", "b", "chi2", "counts", "row", "e"):
            assert got[key].tobytes() == again[key].tobytes(), key
        same_linearisation(m.register(cloud, R, t, 0, **params), want, per_point=False)   # (no per-point buffer: the same sums)
    assert everything(m) == before


@pytest.mark.parametrize("params", [A.DEFAULT, A.GATED], ids=["neutral", "gated"])
def test_five_traced_rounds(corner, twin, params):
    m, (rows, keys, surfels) = corner
    R0, t0 = A.start_pose()
    cloud = A.scan(4097)
    before = everything(m)
    got = m.register(cloud, R0, t0, 5, **params)
    assert everything(m) == before
    assert np.array_equal(got["X"][0], np.concatenate([R0.reshape(-1), t0]))
    c = 8.0 * G.rho_ref()
    for k in range(6):
        Rk, tk = got["X"][k][:9].reshape(3, 3), got["X"][k][9:]
        same_linearisation(got, A.linearize(rows, keys, surfels, cloud, Rk, tk, **params), k, per_point=False)
        if k < 5:
            Rn, tn = A.step(got["H"][k], got["b"][k], Rk, tk)
            ref = G.step(got["H"][k], got["b"][k], got["X"][k])
            _, _, tol = G.bounds(ref, got["X"][k], c)
            err = np.abs(got["X"][k + 1] - np.concatenate([Rn.reshape(-1), tn]))
            print("round %d: chi2 %.6g inliers %d, X_next within %.3f of its tolerance" % (k, got["chi2"][k], got["counts"][k][3], (err / tol).max()))
            assert np.all(err <= tol), (k, (err / tol).max())
    assert np.array_equal(got["X"][5], np.concatenate([got["R"].reshape(-1), got["t"]]))
    assert not np.array_equal(got["X"][1], got["X"][0]) and got["chi2"][1] < got["chi2"][0]
    host = capi.host_map_register(twin, cloud, R0, t0, 5, **params)
    dt, da = A.pose_distance(got["R"], got["t"], host["R"], host["t"])
    assert dt <= 1e-5 and da <= 1e-5, (dt, da)
    assert np.array_equal(got["counts"], host["counts"])
    again = m.register(cloud, R0, t0, 5, **params)
    for key in ("R", "t", "X", "H", "b", "chi2", "counts"):
        assert got[key].tobytes() == again[key].tobytes(), key
    for its in (1, 2):                                                   # (fewer rounds: the first rows of the same run)
        short = m.register(cloud, R0, t0, its, **params)
        assert short["X"].tobytes() == got["X"][:its + 1].tobytes() and short["H"].tobytes() == got["H"][:its + 1].tobytes()


def test_large_cloud_rounds(corner):
    """65 793 points: two join launches per round (257 rows, then 2, then 1)"""
    m, (rows, keys, surfels) = corner
    R0, t0 = A.start_pose()
    cloud = A.scan(65793)
    got = m.register(cloud, R0, t0, 2, **A.GATED)
    for k in range(3):
        same_linearisation(got, A.linearize(rows, keys, surfels, cloud, got["X"][k][:9].reshape(3, 3), got["X"][k][9:], **A.GATED), k, per_point=False)


@pytest.mark.parametrize("kind", [(True, None), (False, (2, 1, 6)), (True, (2, 1, 6))], ids=["attr", "ev", "attr+ev"])
def test_maps_with_other_columns_and_after_removals(ctx, kind):
    R, t = A.start_pose()
    cloud = A.scan(1025)
    m = dev_map(ctx, A.map_folds(), with_attr=kind[0], evidence=kind[1], initial_rows=64)   # (64 rows: the folds grow the block)
    try:
        same_linearisation(m.register(cloud, R, t, 0, per_point=True, **A.GATED), A.linearize(*columns(m), cloud, R, t, **A.GATED))
        rows_before = ctx.map_size(m.mid)
        ctx.map_prune(m.mid, A.CORNER + 2.0, 4.0)
        origin = A.CORNER + 1.5
        cid = ctx.cloud_upload(np.ascontiguousarray(origin + (A.corner_points(600, 9) - origin) * 1.5))
        try:
            ctx.map_clear_rays(m.mid, cid, *EYE, origin)
        finally:
            ctx.cloud_release(cid)
        m.insert(A.corner_points(3000, 10), *EYE)
        assert ctx.map_size(m.mid) != rows_before
        before = everything(m)
        same_linearisation(m.register(cloud, R, t, 0, per_point=True, **A.GATED), A.linearize(*columns(m), cloud, R, t, **A.GATED))
        got = m.register(cloud, R, t, 3, **A.GATED)
        same_linearisation(got, A.linearize(*columns(m), cloud, got["R"], got["t"], **A.GATED), 3, per_point=False)
        assert everything(m) == before
    finally:
        m.close()


def test_empty_map(ctx):
    R, t = A.start_pose()
    m = dev_map(ctx)
    try:
        for its in (0, 3):
            got = m.register(A.scan(257), R, t, its)
            assert np.array_equal(got["counts"], np.tile(np.array([257, 0, 0, 0], np.uint64), (its + 1, 1)))
            assert not got["H"].any() and not got["b"].any() and not got["chi2"].any()
            assert np.array_equal(got["R"], R) and np.array_equal(got["t"], t)
        got = m.register(A.scan(65), R, t, 0, per_point=True)
        assert np.array_equal(got["row"], np.full(65, -1, np.int32)) and not got["e"].any()
    finally:
        m.close()


def test_refusals(ctx, corner):
    m, _ = corner
    L = capi.hip_lib()
    R, t = (np.ascontiguousarray(v) for v in A.start_pose())
    cid = ctx.cloud_upload(np.ascontiguousarray(A.scan(65)))
    plain = ctx.map_create(A.VOXEL, 64, 1 << 20)
    dp = C.POINTER(C.c_double)
    out_R, out_t, trace, counts = np.full(9, 7.0), np.full(3, 7.0), np.full((65, 40), 7.0), np.full((65, 4), 7, np.uint64)
    row, e = np.full(65, 7, np.int32), np.full(65, 7.0)

    def call(h=ctx._h, mid=m.mid, cloud=cid, R_=R, t_=t, params=None, its=0, oR=out_R, ot=out_t, tr=trace, cn=counts, rw=None, ee=None, cap=65,
             **change):
        p = capi.MapAlignParams(**dict(dict(reach=1, max_dist=float("inf"), rho=float("inf"), min_count=3, flat=1.0), **change))
        ptr = lambda a, ct: a.ctypes.data_as(ct) if a is not None else None
        return L.madicp_map_register_cloud(h, mid, cloud, ptr(R_, dp), ptr(t_, dp), None if params == "null" else C.byref(p), its, ptr(oR, dp),
                                           ptr(ot, dp), ptr(tr, dp), ptr(cn, C.POINTER(C.c_uint64)), ptr(rw, C.POINTER(C.c_int32)),
                                           ptr(ee, dp), cap)

    try:
        before = everything(m)
        bad_R, bad_t = R.copy(), t.copy()
        bad_R[0, 1], bad_t[2] = np.nan, np.inf
        refused = [dict(h=None), dict(R_=None), dict(t_=None), dict(params="null"), dict(oR=None), dict(ot=None), dict(tr=None), dict(cn=None),
                   dict(mid=987654), dict(cloud=987654), dict(mid=plain), dict(R_=bad_R), dict(t_=bad_t), dict(reach=2), dict(reach=-1),
                   dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(rho=0.0), dict(rho=-1.0), dict(rho=float("nan")), dict(min_count=2),
                   dict(flat=0.0), dict(flat=1.5), dict(flat=float("nan")), dict(its=-1), dict(its=65), dict(its=1, rw=row), dict(its=1, ee=e)]
        for kw in refused:
            assert call(**kw) == INVALID, kw
        assert call(rw=row, cap=64) == CAPACITY and call(ee=e, cap=64) == CAPACITY
        assert np.all(out_R == 7.0) and np.all(out_t == 7.0) and np.all(trace == 7.0) and np.all(counts == 7)   # nothing written
        assert np.all(row == 7) and np.all(e == 7.0)
        assert call(its=64) == 0 and np.all(counts[:, 0] == 65)          # (the last legal round count)
        assert everything(m) == before
    finally:
        ctx.map_release(plain)
        ctx.cloud_release(cid)
