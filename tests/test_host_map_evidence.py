"""The host twin's evidence column (madicp_host_map_create_ev / _download_evidence / _download_min_evidence, csrc/host/voxel_map.h)
against the numpy restatement of tests/map_evidence_ref.py after EVERY step of mixed sequences of folds, clearings and prunes:
answers, rows, stored keys, words, evidence, the log's count and what a take returns, bit for bit — and the rule's corners one by
one: 1/1/1 is the plain map, a voxel is hit once per fold, saturation, the boundary e == miss, traversed and occupied, decrements
without a removal, the word through a prune and through growths, with the attribute column and the removal log, every refusal, and
the filtered download at its four thresholds.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_evidence_ref as Ev
import map_removed_ref as Rm
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)
from test_host_map_removed import CAPACITY, INVALID, TWIN

_fp, _u64p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@pytest.fixture
def twins(maps):
    """params None: a plain map"""
    return lambda params, **k: maps.host(**{**TWIN, "voxel": Ev.VOXEL, "evidence": params, **k})


def evidence_after(name, params, step=-1):
    return Ev.expected(name, params)[1][step][4]


@pytest.mark.parametrize("params", Ev.PARAMS)
@pytest.mark.parametrize("name", Ev.MIXED_NAMES)
def test_mixed_sequences(twins, name, params):
    done, want = Ev.expected(name, params)
    Ev.replay(done, want, twins(params, initial_rows=1), twins(params, with_attr=False), tag=name, cap=params[2])


@pytest.mark.parametrize("name", Ev.ROW_NAMES + ["growths", "prune_in_front", "old_and_new", "one_voxel"])
def test_named_sequences(twins, name):
    done, want = Ev.expected(name, (2, 3, 9))
    Ev.replay(done, want, twins((2, 3, 9), initial_rows=1), tag=name, cap=9)


@pytest.mark.parametrize("name", Ev.PLAIN_NAMES + Ev.MIXED_NAMES)
def test_one_one_one_is_the_plain_map(twins, name):
    """hit = miss = cap = 1: rows, keys, counts, watermarks and log entries of a plain map driven by the same sequence"""
    steps = Rm.with_takes(Ev.named(name), "every")
    done, want = Ev.run_ref(steps, (1, 1, 1))
    plain_done, plain = Rm.run_ref(steps)
    assert len(done) == len(plain_done)
    for a, b in zip(want, plain):  # the restatements agree step by step ...
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[5] == b[4]
        assert np.all(a[4] == 1)
        assert (a[6] is None) == (b[5] is None) and (a[6] is None or Rm.same_log(a[6], b[5], True))
    Ev.replay(done, want, twins((1, 1, 1), initial_rows=1), twins(None, initial_rows=1), tag=name, cap=1)  # ... and so do the maps


def test_4096_points_in_one_voxel_add_hit_once(twins):
    done, want = Ev.expected("one_voxel", (3, 1, 100))
    Ev.replay(done, want, twins((3, 1, 100)))
    assert [w[4].tolist() for w in want] == [[3, 3], [6, 3], [9, 3]]


def test_old_and_new_voxels_in_one_fold(twins):
    done, want = Ev.expected("old_and_new", (2, 1, 100))
    Ev.replay(done, want, twins((2, 1, 100)))
    assert want[1][4].tolist() == [2] * 10 + [4] * 10 + [2] * 10  # untouched | old and hit (the repeated points: still once) | new


def test_saturation_is_exact(twins):
    I, z = E.IDENTITY
    steps = [("fold", E.own_cells(5), I, z)] * 6
    done, want = Ev.run_ref(steps, (3, 1, 10))
    Ev.replay(done, want, twins((3, 1, 10)), cap=10)
    assert [int(w[4][0]) for w in want] == [3, 6, 9, 10, 10, 10]
    done, want = Ev.run_ref(steps[:3], (5, 1, 5))  # cap == hit: saturated from the first fold on
    Ev.replay(done, want, twins((5, 1, 5)), cap=5)
    assert [int(w[4][0]) for w in want] == [5, 5, 5]
    top = Ev.CAP_MAX
    done, want = Ev.run_ref(steps[:3], (top - 1, 1, top))  # the largest cap: e + hit needs the 32nd bit
    Ev.replay(done, want, twins((top - 1, 1, top)), cap=top)
    assert [int(w[4][0]) for w in want] == [top - 1, top, top]


def test_the_boundary_e_equals_miss_leaves(twins):
    # hit 3, miss 3: e == miss -> voxels 1 .. 3 leave at once; 4 (traversed AND occupied), 5 and 6 (not reached) are unchanged
    done, want = Ev.run_ref(Ev.see_through(1), (3, 3, 9))
    Ev.replay(done, want, twins((3, 3, 9)), cap=9)
    assert want[1][0] == (3, 3, 0) and want[1][4].tolist() == [3, 3, 3]
    # hit 4, miss 3: e == miss + 1 -> they stay with 1, nothing is removed — the decrements are applied all the same; then they leave
    done, want = Ev.run_ref(Ev.see_through(2), (4, 3, 9))
    Ev.replay(done, want, twins((4, 3, 9)), cap=9)
    assert want[1][0] == (0, 6, 3) and want[1][4].tolist() == [1, 1, 1, 4, 4, 4]
    assert want[2][0] == (3, 3, 0) and want[2][4].tolist() == [4, 4, 4]
    assert want[2][6] is None and want[2][5] == 3  # the three left from below the watermark: logged


def test_decrements_without_a_removal_and_hits_in_between(twins):
    I, z = E.IDENTITY
    s = Ev.see_through(2, hits=3)  # e = 6 | miss 2 twice -> 2, nothing ever removed
    s = s + [("fold", Ev.line([2]), I, z)] + s[-1:] * 2  # voxel 2 is hit (4), then two more clearings: 1 and 3 leave, 2 stays with 2
    done, want = Ev.run_ref(s, (2, 2, 6))
    Ev.replay(done, want, twins((2, 2, 6), initial_rows=1), cap=6)
    assert [w[0] for w in want[3:5]] == [(0, 6, 3), (0, 6, 3)]
    assert want[4][4].tolist() == [2, 2, 2, 6, 6, 6] and want[5][4].tolist() == [2, 4, 2, 6, 6, 6]
    assert want[6][0] == (2, 4, 1) and want[6][4].tolist() == [2, 6, 6, 6]
    assert want[7][0] == (1, 3, 2) and want[7][4].tolist() == [6, 6, 6]


def test_the_word_follows_its_row_through_a_prune(twins):
    done, want = Ev.expected("prune_in_front", (1, 1, 5))
    Ev.replay(done, want, twins((1, 1, 5)), cap=5)
    assert want[3][4].tolist() == [1] * 300 + [3, 1, 2, 1] * 75
    assert want[4][0][0] >= 300 and want[4][4].tolist()[:8] == [3, 1, 2, 1, 3, 1, 2, 1]  # the near rows in front are gone


def test_growths_from_one_row(twins):
    done, want = Ev.expected("growths", (1, 1, 4))
    Ev.replay(done, want, twins((1, 1, 4), initial_rows=1), twins((1, 1, 4), initial_rows=1 << 14, with_attr=False), tag="growths", cap=4)
    assert sorted(set(want[-1][4].tolist())) != [1]


def test_with_the_column_and_the_log_and_a_reset(twins):
    steps = Ev.mixed(257) + [("reset",)] + Ev.mixed(65)
    done, want = Ev.run_ref(Rm.with_takes(steps, "every"), (2, 1, 5))
    assert sum(w[6][0].shape[0] for w in want if w[6] is not None) > 0
    Ev.replay(done, want, twins((2, 1, 5), initial_rows=1), cap=5)
    done, want = Ev.run_ref(steps, (2, 1, 5), tracking=False)
    Ev.replay(done, want, twins((2, 1, 5), tracking=False, with_attr=False), cap=5)


def test_download_min_evidence_thresholds(twins):
    done, want = Ev.expected("prune_in_front", (1, 1, 3))
    m = twins((1, 1, 3))
    Ev.replay(done, want, m)
    rows, keys, words, ev = want[-1][1], want[-1][2], want[-1][3], want[-1][4]
    n = rows.shape[0]
    sat = int(np.count_nonzero(ev == 3))
    assert 0 < sat < n
    for min_e, count in [(0, n), (1, n), (3, sat), (4, 0)]:
        got = m.confirmed(min_e)
        assert got[0].shape[0] == count and Ev.same_confirmed(got, rows, keys, words, ev, min_e, True)
    only = capi.host_map_download_min_evidence(m.h, 2)
    assert len(only) == 1 and E.same_bits(only[0], np.ascontiguousarray(rows[ev >= 2]))


def test_refusals(natives):
    L = capi.host_lib()
    h = C.c_void_p()
    for hit, miss, cap in [(0, 1, 1), (1, 0, 1), (2, 1, 1), (1, 1, 2 ** 31), (0, 0, 0), (2 ** 31, 1, 2 ** 32 - 1)]:
        assert Ev.refused(hit, miss, cap)
        assert L.madicp_host_map_create_ev(0.5, 1, 100, 0, hit, miss, cap, C.byref(h)) == INVALID and not h
    assert L.madicp_host_map_create_ev(0.0, 1, 100, 0, 1, 1, 1, C.byref(h)) == INVALID and not h
    assert L.madicp_host_map_create_ev(0.5, 1, 100, 0, 1, 1, 1, None) == INVALID
    I, z = E.IDENTITY
    n = C.c_int64(-7)
    xyz, ev, keys = np.full((8, 3), 7.0, np.float32), np.full(8, 77, np.uint32), np.full(8, 77, np.uint64)
    for make in (capi.host_map_create, capi.host_map_create_attr):  # the downloads on a plain map
        p = make(0.5, 1, 100)
        capi.host_map_insert(p, E.own_cells(4), I, z)
        assert L.madicp_host_map_download_evidence(p, 0, ev.ctypes.data_as(_u32p), 8, C.byref(n)) == INVALID
        assert L.madicp_host_map_download_min_evidence(p, 0, xyz.ctypes.data_as(_fp), None, None, None, 8, C.byref(n)) == INVALID
        assert n.value == -7 and np.all(ev == 77) and np.all(xyz == 7.0)
        capi.host_map_destroy(p)
    m = capi.host_map_create_ev(0.5, 1, 100, 2, 1, 4)
    capi.host_map_insert(m, E.own_cells(6), I, z)
    capi.host_map_insert(m, E.own_cells(3), I, z)
    # short buffers: *out_n is set, nothing is written
    assert L.madicp_host_map_download_evidence(m, 1, ev.ctypes.data_as(_u32p), 4, C.byref(n)) == CAPACITY and n.value == 5
    assert L.madicp_host_map_download_min_evidence(m, 3, xyz.ctypes.data_as(_fp), keys.ctypes.data_as(_u64p), None, ev.ctypes.data_as(_u32p),
                                                   2, C.byref(n)) == CAPACITY and n.value == 3
    assert np.all(ev == 77) and np.all(xyz == 7.0) and np.all(keys == 77)
    # exactly the reported size is enough
    assert L.madicp_host_map_download_min_evidence(m, 3, xyz.ctypes.data_as(_fp), None, None, ev.ctypes.data_as(_u32p), 3, C.byref(n)) == 0
    assert n.value == 3 and ev[:3].tolist() == [4, 4, 4] and ev[3] == 77
    # null arguments, a first_row beyond the rows, an attribute asked of a map without that column
    assert L.madicp_host_map_download_evidence(m, 7, ev.ctypes.data_as(_u32p), 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_evidence(m, 0, None, 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_evidence(m, 0, ev.ctypes.data_as(_u32p), 8, None) == INVALID
    assert L.madicp_host_map_download_min_evidence(m, 0, None, None, None, None, 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_min_evidence(m, 0, xyz.ctypes.data_as(_fp), None, ev.ctypes.data_as(_u32p), None, 8, C.byref(n)) == INVALID
    assert L.madicp_host_map_download_evidence(None, 0, ev.ctypes.data_as(_u32p), 8, C.byref(n)) == INVALID
    assert capi.host_map_download_evidence(m).tolist() == [4, 4, 4, 2, 2, 2]  # ... and nothing of it changed the map
    capi.host_map_clear(m)
    assert L.madicp_host_map_download_min_evidence(m, 0, xyz.ctypes.data_as(_fp), None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    capi.host_map_destroy(m)
