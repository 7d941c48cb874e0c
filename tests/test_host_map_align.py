"""The host twin's registration against the map's surfels (madicp_host_map_register, csrc/host/voxel_map.h: VoxelMap::align) against
the numpy restatement (tests/map_align_ref.py) fed the twin's OWN surfels: counts, per-point row and e exactly equal, H, b, chi2 equal
by value at every size around a wavefront, a workgroup and the tree's second and third level; both reaches, with and without the
robust kernel, every gate one at a time, the empty map, the empty cloud, every refusal; the step of every round within
tests/test_gpu_gn_step.py's tolerance of the restatement's, the final pose within 1e-5 m / 1e-5 rad.  The restatement's Jacobian is
held to central finite differences, and the committed seed to its gate margins.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import gn_step_ref as G
import map_align_ref as A
from mad_icp_amd import capi

INVALID, CAPACITY = -1, -4
MAX_COUNT = 1 << 20


def make_map(folds, with_attr=False, evidence=None):
    h = capi.host_map_create_mom(A.VOXEL, 64, 1 << 22, MAX_COUNT, with_attr=with_attr, evidence=evidence)
    for pts in folds:
        capi.host_map_insert(h, pts, np.eye(3), np.zeros(3))
    return h


def columns(h):
    return capi.host_map_download_f32(h), capi.host_map_download_keys(h), capi.host_map_download_surfels(h)


@pytest.fixture(scope="module")
def corner():
    h = make_map(A.map_folds())
    yield h, columns(h)
    capi.host_map_destroy(h)


def same_linearisation(got, want, k=0, per_point=True):
    assert np.array_equal(got["counts"][k], want["counts"]), (got["counts"][k], want["counts"])
    if per_point:
        assert got["row"].dtype == np.int32 and np.array_equal(got["row"], want["row"])
        assert got["e"].tobytes() == want["e"].tobytes()
    assert np.array_equal(got["H"][k], want["H"]) and np.array_equal(got["b"][k], want["b"]) and got["chi2"][k] == want["chi2"]


def test_most_rows_of_the_scene_have_a_normal(corner):
    _, (rows, keys, surfels) = corner
    assert rows.shape[0] > 400 and np.mean(surfels[3] >= 3) > 0.9


def test_restatement_jacobian_matches_finite_differences(corner):
    _, (rows, keys, surfels) = corner
    R, t = A.start_pose()
    cloud = A.scan(257)
    lin = A.linearize(rows, keys, surfels, cloud, R, t)
    hit = lin["inlier"]
    assert hit.sum() > 200
    J, fd = A.jacobian_fd(surfels, lin["row"][hit], cloud[hit], R, t)
    assert np.abs(J[:, :3]).max() > 0.5 and np.abs(J[:, 3:]).max() > 0.5
    assert np.allclose(J, fd, rtol=0, atol=1e-7), np.abs(J - fd).max()


def test_tree_is_not_a_running_sum():
    x = np.random.default_rng(3).normal(size=(5, A.TERMS)) * np.array([1e16, 1.0, -1e16, 1.0, 1.0])[:, None]
    want = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + 0.0) + 0.0)
    assert np.array_equal(A.tree(x), want) and not np.array_equal(A.tree(x), np.cumsum(x, axis=0)[-1])
    assert np.array_equal(A.tree(x[:1]), x[0]) and not A.tree(x[:0]).any()


@pytest.mark.parametrize("n", A.SIZES)
def test_linearise_only_is_the_restatement(corner, n):
    h, (rows, keys, surfels) = corner
    R, t = A.start_pose()
    cloud = A.scan(n)
    for params in (A.DEFAULT, A.GATED, dict(A.GATED, reach=0)):
        want = A.linearize(rows, keys, surfels, cloud, R, t, **params)
        got = capi.host_map_register(h, cloud, R, t, 0, per_point=True, **params)
        same_linearisation(got, want)
        assert np.array_equal(got["R"], R) and np.array_equal(got["t"], t) and np.array_equal(got["X"][0], np.concatenate([R.reshape(-1), t]))
        same_linearisation(capi.host_map_register(h, cloud, R, t, 0, **params), want, per_point=False)
    if n >= 255:
        assert want["counts"][3] > 0 and want["counts"][3] < want["counts"][1]  # (inliers: some, not all)


def test_every_gate_one_at_a_time(corner):
    h, (rows, keys, surfels) = corner
    R, t = A.start_pose()
    cloud = A.scan(4097)
    base = A.linearize(rows, keys, surfels, cloud, R, t, **A.DEFAULT)
    seen = {}
    for name, change in (("reach", dict(reach=0)), ("max_dist", dict(max_dist=0.25)), ("rho", dict(rho=0.03)), ("min_count", dict(min_count=75)),
                         ("flat", dict(flat=0.02)), ("max_dist-0", dict(max_dist=0.0))):
        params = dict(A.DEFAULT, **change)
        want = A.linearize(rows, keys, surfels, cloud, R, t, **params)
        same_linearisation(capi.host_map_register(h, cloud, R, t, 0, per_point=True, **params), want)
        seen[name] = want
    assert np.any(seen["reach"]["row"] != base["row"])                                       # a neighbour voxel's row was nearer
    assert seen["max_dist"]["counts"][2] < base["counts"][2] and seen["max_dist"]["counts"][1] == base["counts"][1]
    assert np.array_equal(seen["rho"]["counts"], base["counts"]) and 0 < seen["rho"]["chi2"] < base["chi2"]   # the kernel damps, gates nothing
    assert np.any(np.abs(base["e"]) > 0.03)
    for name in ("min_count", "flat"):
        assert 0 < seen[name]["counts"][3] < base["counts"][3] and np.array_equal(seen[name]["counts"][:3], base["counts"][:3]), name
    assert seen["max_dist-0"]["counts"][2] == 0 and not seen["max_dist-0"]["total"].any()


def test_empty_map_and_empty_cloud(corner):
    h, _ = corner
    R, t = A.start_pose()
    empty = capi.host_map_create_mom(A.VOXEL, 64, 1 << 20, MAX_COUNT)
    try:
        for its in (0, 3):
            got = capi.host_map_register(empty, A.scan(257), R, t, its)
            assert np.array_equal(got["counts"], np.tile(np.array([257, 0, 0, 0], np.uint64), (its + 1, 1)))
            assert not got["H"].any() and not got["b"].any() and not got["chi2"].any()
            assert np.array_equal(got["R"], R) and np.array_equal(got["t"], t)
        got = capi.host_map_register(empty, A.scan(65), R, t, 0, per_point=True)
        assert np.array_equal(got["row"], np.full(65, -1, np.int32)) and not got["e"].any()
    finally:
        capi.host_map_destroy(empty)
    for its in (0, 2):
        got = capi.host_map_register(h, np.zeros((0, 3)), R, t, its, per_point=its == 0)
        assert not got["counts"].any() and not got["H"].any() and not got["b"].any() and not got["chi2"].any()
        assert np.array_equal(got["R"], R) and np.array_equal(got["t"], t)


def test_five_rounds_follow_the_restatement(corner):
    h, (rows, keys, surfels) = corner
    R0, t0 = A.start_pose()
    cloud = A.scan(4097)
    for params in (A.DEFAULT, A.GATED):
        got = capi.host_map_register(h, cloud, R0, t0, 5, **params)
        c = 8.0 * G.rho_ref()
        for k in range(5):
            Rk, tk = got["X"][k][:9].reshape(3, 3), got["X"][k][9:]
            same_linearisation(got, A.linearize(rows, keys, surfels, cloud, Rk, tk, **params), k, per_point=False)
            Rn, tn = A.step(got["H"][k], got["b"][k], Rk, tk)
            ref = G.step(got["H"][k], got["b"][k], got["X"][k])
            _, _, tol = G.bounds(ref, got["X"][k], c)
            assert np.all(np.abs(got["X"][k + 1] - np.concatenate([Rn.reshape(-1), tn])) <= tol), k
        assert np.array_equal(got["X"][5], np.concatenate([got["R"].reshape(-1), got["t"]]))
        same_linearisation(got, A.linearize(rows, keys, surfels, cloud, got["R"], got["t"], **params), 5, per_point=False)
        assert got["chi2"][1] < got["chi2"][0] and not np.array_equal(got["X"][1], got["X"][0])
        Rr, tr, lins, _ = A.register(rows, keys, surfels, cloud, R0, t0, 5, **params)
        dt, da = A.pose_distance(got["R"], got["t"], Rr, tr)
        assert dt <= 1e-5 and da <= 1e-5, (dt, da)
        assert np.array_equal(got["counts"][5], lins[5]["counts"])
        dt, da = A.pose_distance(got["R"], got["t"], *A.TRUE_POSE)     # (and it is a registration: back at the truth, to the noise)
        assert dt < 0.01 and da < 0.003, (dt, da)


def test_committed_seed_keeps_every_gate_quantity_off_its_threshold(corner):
    """Seed A.SEED: along the five rounds of the gated run at n = 4 097 — the run the device is compared with the twin on — no matched
    point's d2 lies within a relative 1e-3 of max_dist^2 and no matched row's eig0 within 1e-3 of flat * eig1, so last-bit differences
    between the two sides' normals and eigenvalues (and the poses they lead to) cannot flip a gate."""
    _, (rows, keys, surfels) = corner
    _, _, lins, _ = A.register(rows, keys, surfels, A.scan(4097), *A.start_pose(), 5, **A.GATED)
    for k, lin in enumerate(lins):
        d2m, em = A.gate_margins(lin, surfels, A.GATED["max_dist"], A.GATED["flat"])
        assert d2m > 1e-3 and em > 1e-3, (k, d2m, em)


def test_maps_with_other_columns_and_after_removals(corner):
    _, (rows, keys, surfels) = corner
    R, t = A.start_pose()
    cloud = A.scan(1025)
    h = make_map(A.map_folds(), with_attr=True, evidence=(2, 1, 6))
    try:
        got = capi.host_map_register(h, cloud, R, t, 0, per_point=True, **A.GATED)
        same_linearisation(got, A.linearize(rows, keys, surfels, cloud, R, t, **A.GATED))
        capi.host_map_prune(h, A.CORNER + 2.0, 4.0)
        origin = A.CORNER + 1.5
        capi.host_map_clear_rays(h, origin + (A.corner_points(600, 9) - origin) * 1.5, np.eye(3), np.zeros(3), origin)
        capi.host_map_insert(h, A.corner_points(3000, 10), np.eye(3), np.zeros(3))
        moved = columns(h)
        assert moved[0].shape[0] != rows.shape[0]
        same_linearisation(capi.host_map_register(h, cloud, R, t, 0, per_point=True, **A.GATED), A.linearize(*moved, cloud, R, t, **A.GATED))
    finally:
        capi.host_map_destroy(h)


def test_refusals(corner):
    h, _ = corner
    L = capi.host_lib()
    cloud = np.ascontiguousarray(A.scan(65))
    R, t = (np.ascontiguousarray(v) for v in A.start_pose())
    dp = C.POINTER(C.c_double)
    out_R, out_t, trace, counts = np.full(9, 7.0), np.full(3, 7.0), np.full((65, 40), 7.0), np.full((65, 4), 7, np.uint64)
    row, e = np.full(65, 7, np.int32), np.full(65, 7.0)

    def call(map_=h, xyz=cloud, n=65, R_=R, t_=t, params=None, its=0, oR=out_R, ot=out_t, tr=trace, cn=counts, rw=None, ee=None, cap=65, **change):
        p = capi.MapAlignParams(**dict(dict(reach=1, max_dist=float("inf"), rho=float("inf"), min_count=3, flat=1.0), **change))
        ptr = lambda a, ct: a.ctypes.data_as(ct) if a is not None else None
        return L.madicp_host_map_register(map_, ptr(xyz, dp), n, ptr(R_, dp), ptr(t_, dp), None if params == "null" else C.byref(p), its,
                                          ptr(oR, dp), ptr(ot, dp), ptr(tr, dp), ptr(cn, C.POINTER(C.c_uint64)),
                                          ptr(rw, C.POINTER(C.c_int32)), ptr(ee, dp), cap)

    assert call() == 0
    out_R[:], out_t[:], trace[:], counts[:] = 7.0, 7.0, 7.0, 7
    bad_R = R.copy()
    bad_R[0, 1] = np.nan
    bad_t = t.copy()
    bad_t[2] = np.inf
    plain = capi.host_map_create(A.VOXEL, 64, 1 << 20)
    try:
        refused = [dict(map_=None), dict(xyz=None), dict(R_=None), dict(t_=None), dict(params="null"), dict(oR=None), dict(ot=None), dict(tr=None),
                   dict(cn=None), dict(map_=plain), dict(R_=bad_R), dict(t_=bad_t), dict(n=-1), dict(reach=2), dict(reach=-1),
                   dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(rho=0.0), dict(rho=-1.0), dict(rho=float("nan")), dict(min_count=2),
                   dict(flat=0.0), dict(flat=1.5), dict(flat=float("nan")), dict(its=-1), dict(its=65), dict(its=1, rw=row),
                   dict(its=1, ee=e)]
        for kw in refused:
            assert call(**kw) == INVALID, kw
        assert call(rw=row, cap=64) == CAPACITY and call(ee=e, cap=64) == CAPACITY
        assert call(its=64) == 0                                        # (the last legal round count)
        out_R[:], out_t[:], trace[:], counts[:] = 7.0, 7.0, 7.0, 7
        assert call(rw=row, cap=64) == CAPACITY
    finally:
        capi.host_map_destroy(plain)
    assert np.all(out_R == 7.0) and np.all(out_t == 7.0) and np.all(trace == 7.0) and np.all(counts == 7)   # nothing written
    assert np.all(row == 7) and np.all(e == 7.0)
