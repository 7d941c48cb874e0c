"""The device map's moments (madicp_map_create_mom: fe::map_moments behind the rows' scatter, the ten words and the freeze word through
fe::map_compact, map_grow and madicp_map_clear; madicp_map_download_moments / _download_surfels with fe::map_surfels) against BOTH
the numpy / Python-integer restatement of tests/map_moments_ref.py and the host twin, after EVERY step: answers, rows, stored keys,
words, evidence, the log's count, what a take returns and all ten moment words of every row, bit for bit.  Clouds of 1, 63, 64, 65,
257 and 3 000 points; maps one row below, at and one above the 1 024-mark scan tile; a block grown from one row beside one created
large, so that slot_row and the columns survive every growth and rehash; a fold directly behind a prune and behind a clearing; a
table whose probes wrap; 4 096 points in one voxel at w = 65535; the freeze crossing inside a fold; moments with evidence (2, 1, 6);
a moments map against a plain device map; every refusal.  Surfels: centroid and count bit-equal to the host twin's, eigenvalues
within 4 float32 ulps of it, normals modulo sign within 2.4e-7 per component under the gap filter."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_evidence_ref as Ev
import map_moments_ref as Mo
import map_removed_ref as Rm
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps and twins are fixtures)
from test_host_map_moments import twins  # noqa: F401
from test_host_map_removed import CAPACITY, INVALID, TWIN

pytestmark = pytest.mark.gpu

_fp, _u64p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@pytest.fixture
def made(ctx, maps, twins):
    """device map / host twin factories; max_count None: a plain device map"""
    return (lambda max_count, params=None, **k: maps.dev(ctx, **{**TWIN, "voxel": Mo.VOXEL, "max_count": max_count, "evidence": params, **k})), twins


@pytest.mark.parametrize("max_count", [3, 1000])
@pytest.mark.parametrize("name", Ev.MIXED_NAMES)
def test_mixed_sequences(made, name, max_count):
    """clouds of 1 .. 3 000 points; a fold directly behind a clearing and directly behind a prune; a block grown from one row beside
    one created large, with and without the attribute column"""
    dev, twin = made
    done, want = Mo.expected(name, max_count)
    Mo.replay(done, want, dev(max_count, initial_rows=1), dev(max_count, initial_rows=1 << 13, with_attr=False), twin(max_count), tag=name)


@pytest.mark.parametrize("name", Mo.ROW_NAMES)
def test_row_counts_around_the_scan_tile(made, name):
    dev, twin = made
    done, want = Mo.expected(name, 4, (2, 1, 6))
    assert want[0][0][1] == int(name.split(":")[1])  # exactly that many rows under the marks
    Mo.replay(done, want, dev(4, (2, 1, 6), initial_rows=1), twin(4, (2, 1, 6)), tag=name)


@pytest.mark.parametrize("name", ["growths", "prune_in_front", "old_and_new", "one_voxel"])
def test_named_sequences_with_evidence(made, name):
    """moments together with evidence (2, 1, 6): both columns, one slot_row"""
    dev, twin = made
    done, want = Mo.expected(name, 4, (2, 1, 6))
    Mo.replay(done, want, dev(4, (2, 1, 6), initial_rows=1), dev(4, (2, 1, 6), initial_rows=1 << 14, with_attr=False), twin(4, (2, 1, 6)),
              tag=name)


def test_a_table_whose_probes_wrap(made):
    """cap = 64 rows, 128 slots, no growth: 32 keys that run past the last slot"""
    dev, twin = made
    done, want = Mo.run_ref(Mo.wrapping(), 2)
    assert want[0][0] == (32, 32)
    Mo.replay(done, want, dev(2, initial_rows=64, max_rows=64), twin(2, initial_rows=64, max_rows=64))


def test_4096_points_in_one_voxel_at_the_largest_offset(made):
    """contention and the largest words: n = 4096, S1 = 4096 x 65535, S2 = 4096 x 65535^2"""
    dev, twin = made
    done, want = Mo.expected("one_voxel_top", Mo.MAX_COUNT_MAX)
    Mo.replay(done, want, dev(Mo.MAX_COUNT_MAX), dev(Mo.MAX_COUNT_MAX, initial_rows=1), twin(Mo.MAX_COUNT_MAX))
    top = 65535
    assert want[0][7].tolist() == [[4096] + [4096 * top] * 3 + [4096 * top * top] * 6]


def test_the_freeze_crossing_inside_a_fold(made):
    """max_count = 100 and a fold of 4 096 points into one voxel: the row takes all 4 096, then none; and 4, 4, 4 at max_count 5, 4, 1"""
    dev, twin = made
    done, want = Mo.expected("crossing", 100)
    Mo.replay(done, want, dev(100), dev(100, initial_rows=1), twin(100))
    assert [w[7][:, 0].tolist() for w in want] == [[4096, 60], [4096, 120], [4096, 120]]
    for mc, ns in [(5, [4, 8, 8]), (4, [4, 4, 4]), (1, [4, 4, 4])]:
        done, want = Mo.expected("four_four_four", mc)
        Mo.replay(done, want, dev(mc, initial_rows=1), twin(mc))
        assert [int(w[7][0, 0]) for w in want] == ns


@pytest.mark.parametrize("name", ["prune:posed", "clear:size-1025-257", "clear:edges", "mixed:257"])
def test_moments_never_decide_which_rows_exist(made, name):
    """a moments map against a plain device map on the same sequence: identical answers, rows, keys, attribute and log"""
    dev, _ = made
    steps = Rm.with_takes(Mo.named(name), "every")
    done, want = Mo.run_ref(steps, 3)
    Mo.replay(done, want, dev(3, initial_rows=1), dev(None, initial_rows=1), tag=name)


def test_with_the_log_and_a_reset(made):
    dev, twin = made
    steps = Ev.mixed(257) + [("reset",)] + Ev.mixed(65)
    done, want = Mo.run_ref(Rm.with_takes(steps, "every"), 2, (2, 1, 5))
    Mo.replay(done, want, dev(2, (2, 1, 5), initial_rows=1), twin(2, (2, 1, 5)))


def ulps(a, b):
    """the distance of float32 arrays in units in the last place (same-sign finite values)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_surfels_against_the_host_twin(made):
    dev, twin = made
    pts, R, t = Mo.planes()
    d, h = dev(1 << 20, voxel=0.5, with_attr=False, tracking=False), twin(1 << 20, voxel=0.5, with_attr=False, tracking=False)
    for m in (d, h):
        m.insert(pts, R, t, None)
    assert d.moments().tobytes() == h.moments().tobytes()
    (c, nrm, eig, cnt), (hc, hn, he, hcnt) = d.surfels(), h.surfels()
    assert c.dtype == np.float32 and E.same_bits(c, hc) and cnt.dtype == np.uint32 and cnt.tobytes() == hcnt.tobytes()
    assert E.same_bits(c, Mo.centroids(h.moments(), h.keys(), 0.5))
    ok, left_out = Mo.gap_ok(he, hcnt)
    # Eigenvalues: 4 float32 ulps, on EVERY row.  The solver works in fp64 on the matrix scaled to its largest coefficient, so both
    # sides carry an absolute error of a few 2^-52 of w2; an eigenvalue that is zero but for that rounding (a voxel of one, two or
    # three points, collinear points) has no ulps to speak of — its sign is noise — and is held to 1e-9 of w2 instead, 10^6 times
    # the rounding and a hundredth of a float32 ulp of w2.  A noisy plane's smallest eigenvalue is 1e-3 of w2 and more: ulps.
    w2 = np.abs(he[:, 2:3].astype(np.float64))
    real = np.abs(he.astype(np.float64)) >= 1e-9 * w2
    worst_ulps = int(ulps(eig[real], he[real]).max())
    worst_zero = float((np.abs(eig.astype(np.float64) - he) / np.maximum(w2, 1e-300))[~real].max()) if np.any(~real) else 0.0
    worst = float(Mo.sign_free_diff(nrm[ok], hn[ok]).max())
    print("rows %d, compared %d, left out %.4f, eigenvalues %d ulps (%d of %d by ulps, the others %.3e of w2), normals %.3e" %
          (cnt.shape[0], np.count_nonzero(ok), left_out, worst_ulps, np.count_nonzero(real), real.size, worst_zero, worst))
    assert np.count_nonzero(ok) >= 100 and left_out <= 0.10
    assert np.count_nonzero(real[hcnt >= 4]) == 3 * np.count_nonzero(hcnt >= 4)  # (every eigenvalue of a populated voxel: by ulps)
    assert worst_ulps <= 4 and worst_zero <= 1e-9
    assert worst <= 2.4e-7
    assert np.all(nrm[cnt < 3] == 0.0)
    first = cnt.shape[0] // 3  # a window, and null columns
    c2, n2, e2, k2 = d.surfels(first)
    assert E.same_bits(c2, c[first:]) and E.same_bits(n2, nrm[first:]) and E.same_bits(e2, eig[first:]) and k2.tolist() == cnt[first:].tolist()


def test_refusals(ctx):
    L, h = capi.hip_lib(), ctx._h
    mid = C.c_int(-7)
    ev, bad = (C.c_uint32 * 3)(1, 1, 1), (C.c_uint32 * 3)(0, 1, 1)
    for mc in (0, 2 ** 31 + 1, 2 ** 32 - 1):
        assert L.madicp_map_create_mom(h, 0.5, 1, 100, 0, None, mc, C.byref(mid)) == INVALID and mid.value == -7
    assert L.madicp_map_create_mom(h, 0.5, 1, 100, 0, bad, 5, C.byref(mid)) == INVALID and mid.value == -7
    assert L.madicp_map_create_mom(h, 0.0, 1, 100, 0, None, 5, C.byref(mid)) == INVALID
    assert L.madicp_map_create_mom(h, 0.5, 0, 100, 0, ev, 5, C.byref(mid)) == INVALID
    assert L.madicp_map_create_mom(h, 0.5, 1, 100, 0, None, 5, None) == INVALID
    I, z = E.IDENTITY
    n = C.c_int64(-7)
    mom, xyz, cnt = np.full((8, 10), 77, np.uint64), np.full((8, 3), 7.0, np.float32), np.full(8, 77, np.uint32)
    cid6, cid3 = ctx.cloud_upload(E.own_cells(6)), ctx.cloud_upload(E.own_cells(3))
    for p in (ctx.map_create(0.5, 1, 100), ctx.map_create_attr(0.5, 1, 100), ctx.map_create_ev(0.5, 1, 100, 1, 1, 2)):
        ctx.map_insert_cloud(p, cid6, I, z)
        assert L.madicp_map_download_moments(h, p, 0, mom.ctypes.data_as(_u64p), 8, C.byref(n)) == INVALID
        assert L.madicp_map_download_surfels(h, p, 0, xyz.ctypes.data_as(_fp), None, None, None, 8, C.byref(n)) == INVALID
        assert n.value == -7 and np.all(mom == 77) and np.all(xyz == 7.0)
        ctx.map_release(p)
    m = ctx.map_create_mom(0.5, 1, 100, 2 ** 31)  # (the largest max_count is accepted)
    ctx.map_insert_cloud(m, cid6, I, z)
    assert L.madicp_map_download_moments(h, m, 1, mom.ctypes.data_as(_u64p), 4, C.byref(n)) == CAPACITY and n.value == 5
    assert L.madicp_map_download_surfels(h, m, 0, xyz.ctypes.data_as(_fp), None, None, cnt.ctypes.data_as(_u32p), 5,
                                         C.byref(n)) == CAPACITY and n.value == 6
    assert np.all(mom == 77) and np.all(xyz == 7.0) and np.all(cnt == 77)
    assert L.madicp_map_download_surfels(h, m, 2, xyz.ctypes.data_as(_fp), None, None, cnt.ctypes.data_as(_u32p), 4, C.byref(n)) == 0
    assert n.value == 4 and cnt[:4].tolist() == [1] * 4 and cnt[4] == 77 and np.all(xyz[4:] == 7.0)
    assert L.madicp_map_download_moments(h, m, 6, mom.ctypes.data_as(_u64p), 0, C.byref(n)) == 0 and n.value == 0
    assert L.madicp_map_download_moments(h, m, 7, mom.ctypes.data_as(_u64p), 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_moments(h, m, -1, mom.ctypes.data_as(_u64p), 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_moments(h, m, 0, None, 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_moments(h, m, 0, mom.ctypes.data_as(_u64p), 8, None) == INVALID
    assert L.madicp_map_download_surfels(h, m, 0, None, None, None, None, 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_surfels(h, m, 7, xyz.ctypes.data_as(_fp), None, None, None, 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_surfels(h, m, 0, xyz.ctypes.data_as(_fp), None, None, None, 8, None) == INVALID
    assert L.madicp_map_download_moments(h, m + 1000, 0, mom.ctypes.data_as(_u64p), 8, C.byref(n)) == INVALID
    assert ctx.map_download_moments(m)[:, 0].tolist() == [1] * 6  # ... and nothing of it changed the map
    ctx.map_clear(m)
    ctx.map_insert_cloud(m, cid3, I, z)  # cleared: the words are forgotten with the rows
    assert ctx.map_download_moments(m)[:, 0].tolist() == [1] * 3
    ctx.map_release(m)
    ctx.cloud_release(cid6)
    ctx.cloud_release(cid3)
