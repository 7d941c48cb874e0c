"""The host twin's moments (madicp_host_map_create_mom / _download_moments / _download_surfels, csrc/host/voxel_map.h; the rule is
csrc/common/voxel_moments.h's) against the numpy / Python-integer restatement of tests/map_moments_ref.py after EVERY step of mixed
sequences of folds, clearings and prunes: answers, rows, stored keys, words, evidence, the log's count, what a take returns and all
ten moment words of every row, bit for bit — and the rule's corners one by one: the quantisation edges, the freeze, every refusal,
the centroid's bits, and eigenvalues and normals against numpy.linalg.eigh.  No GPU.

Surfel accuracy, measured here on the planted planes (worst component difference of the host twin's normal against
numpy.linalg.eigh's on the fp64 covariance, modulo sign, over the 276 rows with n >= 3, all of which pass the gap filter): 2.98e-8 —
half a float32 ulp at 1, the output's rounding; eigenvalues: 5.73e-8 of the largest.  The test asserts ten times these, 2.98e-7 and
5.73e-7, and that the normals' bound stays below 1e-6."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_evidence_ref as Ev
import map_moments_ref as Mo
import map_removed_ref as Rm
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)
from test_host_map_removed import CAPACITY, INVALID, TWIN

_fp, _u64p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

# measured on this suite's planes (the module docstring)
MEASURED_NORMAL = 2.98e-8
MEASURED_EIG_REL = 5.73e-8


@pytest.fixture
def twins(maps):
    return lambda max_count, params=None, **k: maps.host(**{**TWIN, "voxel": Mo.VOXEL, "max_count": max_count, "evidence": params, **k})


@pytest.mark.parametrize("max_count", [1, 3, 1000])
@pytest.mark.parametrize("name", Ev.MIXED_NAMES)
def test_mixed_sequences(twins, name, max_count):
    done, want = Mo.expected(name, max_count)
    Mo.replay(done, want, twins(max_count, initial_rows=1), twins(max_count, with_attr=False), tag=name)


@pytest.mark.parametrize("name", Mo.ROW_NAMES + ["growths", "prune_in_front", "old_and_new", "one_voxel", "wrapping"])
def test_named_sequences_with_evidence(twins, name):
    done, want = Mo.expected(name, 4, (2, 1, 6))
    Mo.replay(done, want, twins(4, (2, 1, 6), initial_rows=1), tag=name)


def test_with_the_log_and_a_reset(twins):
    steps = Ev.mixed(257) + [("reset",)] + Ev.mixed(65)
    done, want = Mo.run_ref(Rm.with_takes(steps, "every"), 2)
    Mo.replay(done, want, twins(2, initial_rows=1))
    assert sum(w[6][0].shape[0] for w in want if w[6] is not None) > 0


def test_the_largest_words(twins):
    done, want = Mo.expected("one_voxel_top", Mo.MAX_COUNT_MAX)
    Mo.replay(done, want, twins(Mo.MAX_COUNT_MAX))
    top = 65535
    assert want[0][7].tolist() == [[4096] + [4096 * top] * 3 + [4096 * top * top] * 6]


def test_the_freeze(twins):
    done, want = Mo.expected("four_four_four", 5)
    Mo.replay(done, want, twins(5))
    assert [int(w[7][0, 0]) for w in want] == [4, 8, 8]  # 4 < 5: the second fold is taken whole; 8 >= 5: the third not at all
    assert want[1][7].tobytes() == want[2][7].tobytes()
    done, want = Mo.expected("four_four_four", 1)  # max_count = 1: the creating fold only — all FOUR of its points
    Mo.replay(done, want, twins(1))
    assert [int(w[7][0, 0]) for w in want] == [4, 4, 4]
    done, want = Mo.expected("four_four_four", 4)  # n == max_count at the end of a fold: frozen
    Mo.replay(done, want, twins(4))
    assert [int(w[7][0, 0]) for w in want] == [4, 4, 4]
    done, want = Mo.expected("crossing", 100)
    Mo.replay(done, want, twins(100), twins(100, initial_rows=1))
    assert [w[7][:, 0].tolist() for w in want] == [[4096, 60], [4096, 120], [4096, 120]]


def test_quantisation_edges(twins):
    """q exactly on a cell boundary (w = 0), q = -1e-20 (the quotient rounds so that u is 1.0: w = 65535, in cell -1), both ends of
    the key range, and NaN / out-of-range rows, which contribute nothing"""
    I, z = E.IDENTITY
    v = Mo.VOXEL
    lo, hi = -(2 ** 20) * v, (2 ** 20) * v
    pts = np.array([[1.5, 2.0, -3.5],                      # on a boundary on every axis
                    [-1e-20, -1e-20, -1e-20],              # cell -1, w = 65535
                    [lo, lo, lo],                          # the first cell, w = 0
                    [np.nextafter(hi, 0.0)] * 3,           # the last cell, w = 65535
                    [hi, 0.0, 0.0],                        # one past the range: no candidate
                    [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0],
                    [1.5 + v / 4, 2.0 + v / 2, -3.5 + v / 65536]])  # the first voxel again: 16384, 32768, 1
    done, want = Mo.run_ref([("fold", pts, I, z)], 10)
    Mo.replay(done, want, twins(10))
    mom = want[0][7]
    assert mom.shape[0] == 4
    assert mom[0].tolist() == [2, 16384, 32768, 1, 16384 ** 2, 16384 * 32768, 16384, 32768 ** 2, 32768, 1]
    top = 65535
    assert mom[1].tolist() == [1] + [top] * 3 + [top * top] * 6
    assert mom[2].tolist() == [1] + [0] * 9
    assert mom[3].tolist() == [1] + [top] * 3 + [top * top] * 6
    keys = want[0][2]
    assert [(int(keys[1]) >> (21 * a)) & 0x1fffff for a in range(3)] == [2 ** 20 - 1] * 3
    assert int(keys[2]) == 0 and int(keys[3]) == 2 ** 63 - 1


def test_centroid_bits_and_counts(twins):
    for name, mc in [("mixed:3000", 1000), ("growths", 3), ("one_voxel_top", 10)]:
        done, want = Mo.expected(name, mc)
        m = twins(mc)
        Mo.replay(done, want, m, tag=name)
        keys, mom = want[-1][2], want[-1][7]
        c, nrm, eig, cnt = m.surfels()
        assert c.dtype == np.float32 and E.same_bits(c, Mo.centroids(mom, keys, Mo.VOXEL))
        assert cnt.dtype == np.uint32 and cnt.tolist() == mom[:, 0].tolist()
        assert np.all(nrm[cnt < 3] == 0.0) and np.all(np.isfinite(eig)) and np.all(np.isfinite(nrm))
        first = mom.shape[0] // 2  # a window
        c2, _, _, cnt2 = capi.host_map_download_surfels(m.h, first)
        assert E.same_bits(c2, c[first:]) and cnt2.tolist() == cnt[first:].tolist()
    # the centroid of one point is the middle of its quantisation step
    I, z = E.IDENTITY
    m = twins(10)
    m.insert(np.array([[0.25, 0.0, -0.5]]), I, z, np.zeros(1, np.uint32))
    c, nrm, eig, cnt = m.surfels()
    assert c.tolist() == [[np.float32((32768.5 / 65536) * 0.5), np.float32((0.5 / 65536) * 0.5), np.float32((-1 + 0.5 / 65536) * 0.5)]]
    assert nrm.tolist() == [[0.0, 0.0, 0.0]] and eig.tolist() == [[0.0, 0.0, 0.0]] and cnt.tolist() == [1]


def planes_surfels(twins):
    pts, R, t = Mo.planes()
    m = twins(1 << 20, voxel=0.5, with_attr=False, tracking=False)
    m.insert(pts, R, t, None)
    return m.moments(), m.surfels()


def test_eigenvalues_and_normals_against_eigh(twins):
    """planted noisy planes, rotated off the axes: the host twin's closed-form solve against numpy.linalg.eigh on the fp64 covariance
    formed from the exact integers, modulo sign, over the rows with n >= 3 whose gap w1 - w0 >= 1e-3 w2 — which leaves out at most
    10 % of the rows with n >= 3"""
    mom, (c, nrm, eig, cnt) = planes_surfels(twins)
    want_eig, want_nrm = Mo.eigh_surfels(mom, 0.5)
    ok, left_out = Mo.gap_ok(eig, cnt)
    print("rows %d, n >= 3: %d, compared %d, left out %.4f" % (cnt.shape[0], np.count_nonzero(cnt >= 3), np.count_nonzero(ok), left_out))
    assert np.count_nonzero(ok) >= 100 and left_out <= 0.10
    worst = float(Mo.sign_free_diff(nrm[ok], want_nrm[ok]).max())
    rel = float((np.abs(eig[ok].astype(np.float64) - want_eig[ok]) / want_eig[ok][:, 2:3]).max())
    print("worst normal component difference %.3e, worst eigenvalue difference relative to w2 %.3e" % (worst, rel))
    assert 10 * MEASURED_NORMAL <= 1e-6  # (a bound beyond that would be a finding, not a tolerance)
    assert worst <= 10 * MEASURED_NORMAL
    assert rel <= 10 * MEASURED_EIG_REL
    assert np.allclose(np.linalg.norm(nrm[ok].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_refusals(natives):
    L = capi.host_lib()
    h = C.c_void_p()
    ev = (C.c_uint32 * 3)(1, 1, 1)
    bad = (C.c_uint32 * 3)(0, 1, 1)
    for mc in (0, 2 ** 31 + 1, 2 ** 32 - 1):
        assert Mo.refused(mc)
        assert L.madicp_host_map_create_mom(0.5, 1, 100, 0, None, mc, C.byref(h)) == INVALID and not h
    assert L.madicp_host_map_create_mom(0.5, 1, 100, 0, bad, 5, C.byref(h)) == INVALID and not h
    assert L.madicp_host_map_create_mom(0.0, 1, 100, 0, None, 5, C.byref(h)) == INVALID and not h
    assert L.madicp_host_map_create_mom(0.5, 0, 100, 0, ev, 5, C.byref(h)) == INVALID and not h
    assert L.madicp_host_map_create_mom(0.5, 1, 100, 0, None, 5, None) == INVALID
    I, z = E.IDENTITY
    n = C.c_int64(-7)
    mom, xyz, cnt = np.full((8, 10), 77, np.uint64), np.full((8, 3), 7.0, np.float32), np.full(8, 77, np.uint32)
    plain = [capi.host_map_create(0.5, 1, 100), capi.host_map_create_attr(0.5, 1, 100), capi.host_map_create_ev(0.5, 1, 100, 1, 1, 2)]
    for p in plain:  # the downloads on a map without moments
        capi.host_map_insert(p, E.own_cells(4), I, z)
        assert L.madicp_host_map_download_moments(p, 0, mom.ctypes.data_as(_u64p), 8, C.byref(n)) == INVALID
        assert L.madicp_host_map_download_surfels(p, 0, xyz.ctypes.data_as(_fp), None, None, None, 8, C.byref(n)) == INVALID
        assert n.value == -7 and np.all(mom == 77) and np.all(xyz == 7.0)
        capi.host_map_destroy(p)
    m = capi.host_map_create_mom(0.5, 1, 100, 2 ** 31)  # (the largest max_count is accepted)
    capi.host_map_insert(m, E.own_cells(6), I, z)
    # short buffers: *out_n is set, nothing is written
    assert L.madicp_host_map_download_moments(m, 1, mom.ctypes.data_as(_u64p), 4, C.byref(n)) == CAPACITY and n.value == 5
    assert L.madicp_host_map_download_surfels(m, 0, xyz.ctypes.data_as(_fp), None, None, cnt.ctypes.data_as(_u32p), 5,
                                              C.byref(n)) == CAPACITY and n.value == 6
    assert np.all(mom == 77) and np.all(xyz == 7.0) and np.all(cnt == 77)
    # exactly the reported size is enough; the optional columns may be null
    assert L.madicp_host_map_download_surfels(m, 2, xyz.ctypes.data_as(_fp), None, None, cnt.ctypes.data_as(_u32p), 4, C.byref(n)) == 0
    assert n.value == 4 and cnt[:4].tolist() == [1] * 4 and cnt[4] == 77 and np.all(xyz[4:] == 7.0)
    assert L.madicp_host_map_download_moments(m, 6, mom.ctypes.data_as(_u64p), 0, C.byref(n)) == 0 and n.value == 0
    # null arguments, a first_row outside the rows
    assert L.madicp_host_map_download_moments(m, 7, mom.ctypes.data_as(_u64p), 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_moments(m, -1, mom.ctypes.data_as(_u64p), 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_moments(m, 0, None, 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_moments(m, 0, mom.ctypes.data_as(_u64p), 8, None) == INVALID
    assert L.madicp_host_map_download_surfels(m, 0, None, None, None, None, 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_surfels(m, 7, xyz.ctypes.data_as(_fp), None, None, None, 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_surfels(m, 0, xyz.ctypes.data_as(_fp), None, None, None, 8, None) == INVALID
    assert L.madicp_host_map_download_moments(None, 0, mom.ctypes.data_as(_u64p), 8, C.byref(n)) == INVALID
    assert capi.host_map_download_moments(m)[:, 0].tolist() == [1] * 6  # ... and nothing of it changed the map
    capi.host_map_clear(m)
    capi.host_map_insert(m, E.own_cells(3), I, z)  # cleared: the words are forgotten with the rows
    assert capi.host_map_download_moments(m)[:, 0].tolist() == [1] * 3
    capi.host_map_destroy(m)
