"""The device scan front-end (madicp_cloud_upload / _ingest_f32 / _cloud_deskew, mad_icp_amd/csrc/hip/frontend.hip.h) where
dense inputs do not reach: lagging walks and the three carries of the deskew's prefix minimum, the ends of the threshold table,
azimuths next to a threshold, compaction at tile multiples and past one strip of tile sums, norms on the range bounds, the
float upload's tail, split and hand-over.

deskew  — row for row against the oracle's Pipeline::deskew (oracle_lib.deskew), and the time chunks against the literal walk
          of tests/deskew_ref.py (held to the oracle on the CPU by tests/test_deskew_ref.py).  On a dense scan consecutive
          points cross at most one threshold, T_d - d never rises, the prefix minimum is the element itself and none of
          pmin_tiles / pmin_top / the carries of deskew_apply changes a result; every cloud here first asserts FROM THE
          REFERENCE WALK'S CENSUS that it lags where it is meant to, so that a cloud that stopped lagging fails.
ingest  — bitwise (uint64 views: the sign of a zero counts) against oracle_lib.ingest_f32.
upload  — bitwise round trip.
"""
import functools
import math

import numpy as np
import pytest

import deskew_ref as D
import oracle_lib as O
from mad_icp_amd import capi

pytestmark = pytest.mark.gpu


def _pose(tx, ty, yaw, pitch):
    T = np.eye(4)
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T[:3, 3] = [tx, ty, 0.01]
    return T


# the three motions of test_gpu_frontend.py::test_deskew_matches_oracle + a fast yaw (3 rad/s at 10 Hz: neighbouring chunks
# differ by 3e-4 rad, 1 cm at 30 m)
MOTIONS = [(0.9, 0.05, 0.02, 0.03), (0.0, 0.0, 0.0, 0.0), (-1.4, 0.3, -0.2, 0.01), (0.2, 0.0, 0.3, 0.0)]
HZ = 10.0


def device_deskew(ctx, pts, vel):
    cid = ctx.cloud_upload(pts)
    try:
        chunks = ctx.cloud_deskew(cid, vel, HZ, want_chunks=True)
        return ctx.cloud_download(cid), chunks
    finally:
        ctx.cloud_release(cid)


def check_deskew(ctx, pts, w):
    """every motion: the device's rows are the oracle's, its chunks the reference walk's"""
    for motion in MOTIONS:
        ref, vel = O.deskew(pts, np.eye(4), _pose(*motion), HZ)
        out, chunks = device_deskew(ctx, pts, vel)
        assert np.array_equal(chunks, w["chunks"]), (motion, int((chunks != w["chunks"]).sum()))
        assert np.array_equal(out, ref), motion


@functools.lru_cache(maxsize=None)
def straddle(P):
    pts = D.straddle_cloud(P)
    pts.setflags(write=False)
    return pts, D.walk(pts)


# ---- 3. device deskew, exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.SPARSE_SIZES)
@pytest.mark.parametrize("kind", D.SPARSE_KINDS)
def test_deskew_of_small_and_sparse_clouds(ctx, kind, n):
    pts = D.sparse_cloud(kind, n)
    w = D.walk(pts)
    assert w["lagging"] >= 1                                        # the condition: this cloud lags ...
    assert (w["rises"] >= 1) == D.sparse_has_rise(kind, n)          # ... and T_d - d rises (deskew_ref.sparse_has_rise: where it can)
    check_deskew(ctx, pts, w)


@pytest.mark.parametrize("P", sorted(D.STRADDLE_HEADS))
def test_deskew_lagging_across_a_carry(ctx, P):
    """A lag that crosses a wavefront edge (P = 54), a tile edge (724, 3071; 1024: starting exactly at one) and the 256-tile
    strip edge of pmin_top (261 844, n = 266 844)."""
    pts, w = straddle(P)
    width = D.STRADDLE_HEADS[P]
    if P == 1024:  # the lag STARTS at the tile edge: the head does not lag, position 1 024 does, and depends on the head
        assert not w["lag"][1023] and w["lag"][1024] and 1024 in w["live_across"][D.TILE]
    else:
        assert w["lag_across"][width], "the walk no longer lags on both sides of a multiple of %d" % width
    if P != 54:  # what came before the edge decides the chunk behind it (deskew_ref.walk: live_across), at 14+ wavefront edges too
        assert w["live_across"][width] and len(w["live_across"][D.WAVE]) >= 14
    if P == 261844:
        assert w["live_across"][D.STRIP] == [D.STRIP] and w["live_across"][D.TILE] == [D.STRIP]
    check_deskew(ctx, pts, w)


@pytest.mark.parametrize("name", ["last_three_chunks", "minus_pi", "plus_pi"])
def test_deskew_at_the_end_of_the_threshold_table(ctx, name):
    pts = D.table_end_clouds()[name]
    w = D.walk(pts)
    if name == "last_three_chunks":                                  # the walk never catches up
        assert np.array_equal(w["chunks"], np.arange(1, pts.shape[0] + 1))
    else:
        assert abs(w["az"][0 if name == "plus_pi" else -1]) == math.pi
    check_deskew(ctx, pts, w)


def test_deskew_next_to_a_threshold(ctx):
    """About 400 points whose libm azimuth is 1e-12 .. 1e-10 rad below / above a threshold (1e-12 rad is ~2 000 ulp at pi, far
    beyond any double atan2's error), where the walk has caught up: the device must place every one like the reference."""
    pts, near = D.near_threshold_cloud()
    w = D.walk(pts)
    near_walk = near[w["order"]][::-1]
    assert 380 <= near_walk.sum() <= 420 and np.array_equal(w["chunks"][near_walk], w["T"][near_walk])
    check_deskew(ctx, pts, w)


def test_deskew_threshold_census(ctx, capsys):
    """REPORTED, not asserted: how many points closer than 1e-12 rad to a threshold, and exactly on one, the device places in
    another chunk than the reference walk — the measure of "the device atan2 only has to order and place"."""
    lines = []
    for lo, hi in ((1e-13, 1e-12), (1e-14, 1e-13), (1e-15, 1e-14)):
        pts, near = D.near_threshold_cloud(lo=lo, hi=hi)
        w = D.walk(pts)
        _, chunks = device_deskew(ctx, pts, np.zeros(6))
        near_walk = near[w["order"]][::-1]
        lines.append("%.0e .. %.0e rad: %d of %d near points in another chunk (%d of all %d positions)"
                     % (lo, hi, int((chunks != w["chunks"])[near_walk].sum()), int(near_walk.sum()),
                        int((chunks != w["chunks"]).sum()), chunks.size))
    xy = D.on_threshold_points(count=60)
    base, _ = D.near_threshold_cloud()
    pts = np.vstack([base, np.column_stack([xy, np.full(xy.shape[0], 0.25)])])
    az = D.check_distinct(pts)
    on = np.isin(az, D.thresholds())
    w = D.walk(pts)
    _, chunks = device_deskew(ctx, pts, np.zeros(6))
    on_walk = on[w["order"]][::-1]
    lines.append("exactly on a threshold: %d of %d points in another chunk (%d of all %d positions)"
                 % (int((chunks != w["chunks"])[on_walk].sum()), int(on_walk.sum()), int((chunks != w["chunks"]).sum()), chunks.size))
    with capsys.disabled():
        print("\n[device deskew, azimuths next to a chunk threshold]\n  " + "\n  ".join(lines))
    assert chunks.size == pts.shape[0]


def test_deskew_scratch_growth_and_reuse(ctx):
    """266 844 points, then 37, then 1 025 on the session's context (scratch grown by the first, reused by the others: stale
    tile minima and targets of the large cloud lie behind the small ones) and on a fresh context: identical, and the oracle's."""
    clouds = [straddle(261844)[0], D.sparse_cloud("sectors", 37), D.sparse_cloud("bursts", 1025)]
    motion = MOTIONS[3]
    refs = [O.deskew(p, np.eye(4), _pose(*motion), HZ) for p in clouds]
    fresh = capi.Context(0)
    try:
        for p, (ref, vel) in zip(clouds, refs):
            out_a, ch_a = device_deskew(ctx, p, vel)
            out_b, ch_b = device_deskew(fresh, p, vel)
            assert np.array_equal(out_a, out_b) and np.array_equal(ch_a, ch_b)
            assert np.array_equal(out_a, ref) and np.array_equal(ch_a, D.walk(p)["chunks"])
    finally:
        fresh.close()


# ---- 4. ingest, bitwise ------------------------------------------------------------------------------------------------------
def _records(xyz, stride, seed=0):
    rec = np.random.default_rng(seed).normal(size=(xyz.shape[0], stride)).astype(np.float32)   # (the other fields: anything)
    rec[:, :3] = xyz
    return rec


def check_ingest(ctx, rec, min_range, max_range, kitti, expect_kept=None):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):    # (1e20f squared, denormals, inf - inf in dropped records)
        ref = O.ingest_f32(rec, min_range, max_range, kitti)
    if expect_kept is not None:
        assert ref.shape[0] == expect_kept                            # (the reference itself does what the case is built for)
    cid, kept = ctx.cloud_ingest_f32(rec, min_range, max_range, kitti)
    try:
        out = ctx.cloud_download(cid)
    finally:
        ctx.cloud_release(cid)
    assert kept == ref.shape[0] == out.shape[0]
    nan_o, nan_r = np.isnan(out), np.isnan(ref)
    assert np.array_equal(nan_o, nan_r)
    assert np.array_equal(out.view(np.uint64)[~nan_o], ref.view(np.uint64)[~nan_r])
    return out


INGEST_COUNTS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 4096]


def _survivors(pattern, n):
    keep = np.zeros(n, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "alternating":
        keep[::2] = True
    else:  # one per tile of 1024 marks, at another place in every tile
        t = np.arange((n + 1023) // 1024)
        keep[np.minimum(t * 1024 + (37 * t + 5) % 1024, n - 1)] = True
    return keep


def _patterned(keep, seed):
    """records kept where `keep`, dropped elsewhere (below min_range and beyond max_range in turn)"""
    rng = np.random.default_rng(seed)
    n = keep.size
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz = d * rng.uniform(2.0, 60.0, n)[:, None]
    drop = d * np.where(np.arange(n) % 2 == 0, 0.3, 300.0)[:, None]
    return np.where(keep[:, None], xyz, drop).astype(np.float32)


@pytest.mark.parametrize("stride", [3, 4, 5, 9])
@pytest.mark.parametrize("kitti", [0, 1])
def test_ingest_counts_and_survivor_patterns(ctx, kitti, stride):
    for n in INGEST_COUNTS:
        for pattern in ("all", "first", "last", "alternating", "one_per_tile"):
            keep = _survivors(pattern, n)
            rec = _records(_patterned(keep, n), stride)
            out = check_ingest(ctx, rec, 0.7, 120.0, kitti, expect_kept=int(keep.sum()))
            if not kitti:                                             # in input order
                assert np.array_equal(out, rec[keep, :3].astype(np.float64)), (n, pattern)


@pytest.mark.parametrize("stride", [3, 4, 5, 9])
@pytest.mark.parametrize("kitti", [0, 1])
def test_ingest_past_one_strip_of_tile_sums(ctx, kitti, stride):
    """263 169 records = 258 tiles of marks: tb_scan_top carries over its first strip of 256 tile sums.  About one survivor in
    seven; 3 000 dropped records straddle record 262 144."""
    n = 263169
    keep = np.random.default_rng(5).integers(7, size=n) == 0
    keep[260100:263100] = False
    assert keep[:260100].sum() > 30000 and keep[263100:].any() and 260100 < 262144 < 263100
    check_ingest(ctx, _records(_patterned(keep, 6), stride), 0.7, 120.0, kitti, expect_kept=int(keep.sum()))


def _f32_norm(xyz):
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(x * x + (y * y + z * z))


def _on_bound(bound, rng, count):
    """float records whose FLOAT norm is exactly `bound`, one float ulp below and one above (axis points and found ones)"""
    b = np.float32(bound)
    assert float(b) == bound
    cands = [np.array([[b, 0, 0], [0, -b, 0], [0, 0, b], [-0.0, 0, -b]], np.float32)]
    d = rng.normal(size=(40000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    cands.append((d * (bound * (1.0 + rng.uniform(-1.5e-7, 1.5e-7, d.shape[0])))[:, None]).astype(np.float32))
    xyz = np.vstack(cands)
    nrm = _f32_norm(xyz)
    below, above = np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(np.inf))
    out = {}
    for name, v in (("on", b), ("below", below), ("above", above)):
        sel = xyz[nrm == v][:count]
        if name != "on":  # the axis points one ulp away
            axis = np.array([[v, 0, 0], [0, 0, -v]], np.float32)
            assert (_f32_norm(axis) == v).all()
            sel = np.vstack([axis, sel])
        assert sel.shape[0] >= 4, (bound, name)
        out[name] = sel
    return out


@pytest.mark.parametrize("stride", [3, 4, 5, 9])
@pytest.mark.parametrize("kitti", [0, 1])
def test_ingest_range_bounds_and_special_values(ctx, kitti, stride):
    rng = np.random.default_rng(23)
    lo, hi = 0.5, 64.0                                                # exact floats
    at_lo, at_hi = _on_bound(lo, rng, 20), _on_bound(hi, rng, 20)
    kept = [at_lo["on"], at_lo["above"], at_hi["on"], at_hi["below"]]  # the comparisons are strict: ON a bound stays
    dropped = [at_lo["below"], at_hi["above"]]
    f = np.float32
    kept.append(np.array([[1e-40, 3, 4], [3, -1e-45, 4], [-0.0, 3, 4], [3, -0.0, 4], [-0.0, -0.0, 5], [0.0, -0.0, -5], [-0.0, 0.0, 0.5],
                          [-3, -0.0, -0.0]], f))                      # float denormals; -0.0 in x / y, alone and on the z axis
    dropped.append(np.array([[1e20, 0, 0], [0, 1, -1e20], [np.inf, 0, 0], [1, -np.inf, 1], [np.inf, np.inf, -np.inf], [1e-40, 0, 0],
                             [-0.0, -0.0, -0.0], [np.nan, 1, 1], [1, 1, np.nan]], f))  # x*x = inf in float; infinities; |p| = 0
    n_kept = sum(k.shape[0] for k in kept)
    xyz = np.vstack(kept + dropped)
    flag = np.concatenate([np.ones(n_kept, bool), np.zeros(xyz.shape[0] - n_kept, bool)])
    perm = rng.permutation(xyz.shape[0])
    out = check_ingest(ctx, _records(xyz[perm], stride), lo, hi, kitti, expect_kept=n_kept)
    if not kitti:
        assert np.array_equal(out.view(np.uint64), xyz[perm][flag[perm]].astype(np.float64).view(np.uint64))

    # the project's 0.7 / 120.0 (no floats): records whose float norm and double norm fall on different sides of a bound —
    # the float decision is the reference's (Vector3f::norm(), bin_runner.cpp:149)
    found = []
    for bound in (0.7, 120.0):
        d = rng.normal(size=(200000, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        c = (d * (bound * (1.0 + rng.uniform(-2e-7, 2e-7, d.shape[0])))[:, None]).astype(np.float32)
        nf = _f32_norm(c).astype(np.float64)
        c64 = c.astype(np.float64)
        nd = np.sqrt(c64[:, 0] ** 2 + c64[:, 1] ** 2 + c64[:, 2] ** 2)
        for side in (np.less, np.greater):
            sel = c[side(nf, bound) != side(nd, bound)]
            assert sel.shape[0] >= 8, (bound, sel.shape)
            found.append(sel[:40])
    xyz = np.vstack(found + [np.array([[3, 4, 0]], f)])
    nf = _f32_norm(xyz).astype(np.float64)
    check_ingest(ctx, _records(xyz, stride), 0.7, 120.0, kitti, expect_kept=int(((nf >= 0.7) & (nf <= 120.0)).sum()))


# ---- 5. float upload, bitwise round trip -------------------------------------------------------------------------------------
UPLOAD_COUNTS = [1365, 1366, 1367, 1368, 1369, 21845, 21846, 21847, 43691]  # 3n = 4095 (under the float path's threshold of
# 4096 values), every 3n % 4 (the widening kernel's scalar tail), one piece / two pieces of 65 536 values (/ three at 43 691)


def _float_exact(n, seed):
    rng = np.random.default_rng(seed)
    pts = (rng.normal(size=(n, 3)) * [20.0, 15.0, 2.0]).astype(np.float32).astype(np.float64)
    pts[n // 3] = [-0.0, np.inf, -np.inf]
    pts[-1, 2] = -0.0
    return pts


def _round_trip(ctx, pts, what):
    try:
        for opt in (1, 0):
            ctx.set_option("upload_f32", opt)
            cid = ctx.cloud_upload(pts)
            try:
                back = ctx.cloud_download(cid)
            finally:
                ctx.cloud_release(cid)
            assert np.array_equal(back.view(np.uint64), pts.view(np.uint64)), (what, opt)
    finally:
        ctx.set_option("upload_f32", 1)


@pytest.mark.parametrize("n", UPLOAD_COUNTS)
def test_upload_round_trip_at_the_float_path_edges(ctx, n):
    _round_trip(ctx, _float_exact(n, n), "float-exact")
    _round_trip(ctx, np.random.default_rng(n).normal(size=(n, 3)), "genuine doubles")


@pytest.mark.parametrize("n", [21846, 21847, 43691])
def test_upload_hand_over_at_the_first_value_that_is_no_float(ctx, n):
    """the float path stops at the piece that holds the first value that is not exactly a float; what it sent so far is widened
    on the device, the rest goes as doubles: last value of piece one, first of piece two, the very last value"""
    base = _float_exact(n, 100 + n)
    for flat in (65535, 65536, 3 * n - 1):
        for bad in (np.nextafter(1.5, 2.0), np.nan, 1e300):
            pts = base.copy()
            pts.reshape(-1)[flat] = bad
            _round_trip(ctx, pts, (flat, bad))
