"""The host twin's removal log (madicp_host_map_track_removed / _removed_count / _take_removed, csrc/host/voxel_map.h: the append
in VoxelMap::close_up) and its key and row downloads (_download_keys / _download_rows) against the numpy restatement of
tests/map_removed_ref.py after EVERY step of the sequences of tests/map_prune_ref.py and tests/map_clear_ref.py: answers, rows,
stored keys, words, the log's count and what a take returns, bit for bit — taking after every step and only at the end, at the
watermarks 0, 1, M/2, M - 1 and M, with and without the attribute column, tracking off, switched on and off mid-sequence, the
full log, and every refusal with nothing changed.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloud_export_ref as E
import map_clear_ref as Cl
import map_prune_ref as P
import map_removed_ref as Rm
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)
from test_host_map_clear import TWIN

INVALID, CAPACITY = -1, -4
_fp, _u64p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

PRUNE_NAMES = ["prune:" + n for n in P.SIZE_NAMES + P.OTHER_NAMES]
CLEAR_NAMES = ["clear:" + n for n in Cl.SIZE_NAMES + ["edges", "protected", "everything", "but_the_endpoints", "scene"]]
WATERMARK_NAMES = ["prune:size-1025-alternate", "prune:size-4097-median", "prune:size-257-all", "clear:size-1025-257", "clear:but_the_endpoints"]


TWIN = dict(TWIN, tracking=True, refusals=True)  # tests/test_host_map_clear.py's maps with what tests/map_removed_ref.py's replay asks for


@pytest.fixture
def twins(maps):
    return functools.partial(maps.host, **TWIN)


def logged(want):
    """the entries all takes of a replay returned"""
    return sum(w[5][0].shape[0] for w in want if w[5] is not None)


@pytest.mark.parametrize("cadence", ["every", "end"])
@pytest.mark.parametrize("name", PRUNE_NAMES + CLEAR_NAMES)
def test_sequences(twins, name, cadence):
    done, want = Rm.expected(name, cadence)
    Rm.replay(done, want, twins(initial_rows=1), tag=name)
    # the log holds what left from below the watermarks, no more: the sum of watermark - watermark_out over the removals
    assert logged(want) == sum(s[-1] - w[0][2] for s, w in zip(done, want) if s[0] in ("prune", "clear"))


@pytest.mark.parametrize("watermark", Rm.WATERMARKS[1:])
@pytest.mark.parametrize("name", WATERMARK_NAMES)
def test_watermarks(twins, name, watermark):
    done, want = Rm.expected(name, "every", watermark)
    Rm.replay(done, want, twins(), twins(with_attr=False), tag=name)
    n = logged(want)
    removed = sum(w[0][0] for s, w in zip(done, want) if s[0] in ("prune", "clear"))
    assert n == 0 if watermark == "0" else n <= removed
    if watermark == "all":
        assert n == removed > 0  # every row was delivered: every removed row is logged


def test_accumulated_takes_have_a_base(twins):
    """taking only at the end: the three removals of "posed" and of "growth" pile up in one log"""
    for name, removals in (("prune:posed", 3), ("prune:growth", 3)):
        done, want = Rm.expected(name, "end")
        counts = [w[4] for s, w in zip(done, want) if s[0] == "prune"]
        assert len(counts) == removals and all(b > a > 0 for a, b in zip(counts, counts[1:])), counts
        Rm.replay(done, want, twins(initial_rows=1, with_attr=False), tag=name)


def one_then_4097():
    """a first removal that logs ONE row, then one that logs 4097"""
    I, z = E.IDENTITY
    far, cells = np.array([[5000.25, 0.25, 0.25]]), E.own_cells(4097)
    return [("fold", far, I, z), ("fold", cells, I, z), ("prune", np.array([20.0, 20.0, 3.0]), 1000.0, "all"),
            ("prune", np.array([1.0e4, 0.0, 0.0]), 1.0, "all"), ("take",), ("fold", cells, I, z)]


def test_one_row_then_4097(twins):
    done, want = Rm.run_ref(one_then_4097())
    assert [w[4] for w in want] == [0, 0, 1, 4098, 0, 0]
    Rm.replay(done, want, twins(initial_rows=1), twins(initial_rows=1, with_attr=False))


def test_reentry_logs_a_key_twice(twins):
    """"reentry" with every watermark = rows: the removed voxels are filled again by the second fold and leave again — the same keys
    are in the first take and in the second"""
    done, want = Rm.expected("prune:reentry", "every", "all")
    Rm.replay(done, want, twins(), tag="reentry")
    takes = [w[5] for w in want if w[5] is not None and w[5][0].shape[0]]
    assert len(takes) == 2 and takes[0][0].shape[0] > 500
    assert takes[0][0].tobytes() == takes[1][0].tobytes() and takes[0][1].tobytes() == takes[1][1].tobytes()
    for t in takes:
        assert np.unique(t[0]).shape[0] == t[0].shape[0]  # within one poll the keys are distinct


@pytest.mark.parametrize("name", PRUNE_NAMES + CLEAR_NAMES)
def test_tracking_off_changes_nothing(twins, name):
    """not tracking: byte-equal maps and answers to tracking, and the count stays 0"""
    on_done, on = Rm.expected(name, "never")
    off_done, off = Rm.expected(name, "never", tracking=False)
    for a, b in zip(on, off):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
        assert b[4] == 0
    assert on[-1][4] == sum(s[-1] - w[0][2] for s, w in zip(on_done, on) if s[0] in ("prune", "clear"))
    Rm.replay(off_done, off, twins(tracking=False), tag=name)
    Rm.replay(on_done, on, twins(), tag=name)


def test_tracking_switched_mid_sequence(twins):
    steps = P.named("posed")
    steps = steps[:2] + [("track", True)] + steps[2:4] + [("track", False)] + steps[4:] + [("track", True), ("take",)]
    done, want = Rm.run_ref(steps, tracking=False)
    counts = [w[4] for w in want]
    assert counts[:3] == [0, 0, 0] and counts[4] > 0 and counts[5:] == [0] * len(counts[5:])  # off: freed, the count is 0
    Rm.replay(done, want, twins(initial_rows=1, tracking=False))


def test_take_on_a_map_that_does_not_track(twins):
    m = twins(tracking=False)
    keys, rows, n = np.zeros(4, np.uint64), np.zeros((4, 3), np.float32), C.c_int64(-7)
    L = capi.host_lib()
    assert L.madicp_host_map_take_removed(m.h, keys.ctypes.data_as(_u64p), rows.ctypes.data_as(_fp), None, 4, C.byref(n)) == INVALID
    assert n.value == -7 and m.removed_count() == 0


def test_the_log_is_bounded_by_max_rows(twins):
    """max_rows = 64: fold 64, prune all at watermark 64, fold 64 again — the second prune is refused, map and log byte-equal to
    before; after a take it succeeds"""
    I, z = E.IDENTITY
    cells, far = E.own_cells(64), np.array([1.0e4, 0.0, 0.0])
    steps = [("fold", cells, I, z), ("prune", far, 1.0, "all"), ("fold", cells, I, z), ("prune", far, 1.0, "all"),
             ("clear", cells * 1.5, I, z, np.zeros(3), 0.0, "all"), ("take",), ("prune", far, 1.0, "all"), ("take",)]
    done, want = Rm.run_ref(steps, max_rows=64)
    assert [w[0] for w in want] == [(64, 64), (64, 0, 0), (64, 64), None, None, None, (64, 0, 0), None]
    assert [w[4] for w in want] == [0, 64, 64, 64, 64, 0, 64, 0]
    for with_attr in (True, False):
        Rm.replay(done, want, twins(initial_rows=64, max_rows=64, with_attr=with_attr))
    m = twins(initial_rows=64, max_rows=64)  # the refused call writes nothing
    Rm.replay(done[:3], want[:3], m)
    a, b, k = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    c = np.ascontiguousarray(far)
    assert capi.host_lib().madicp_host_map_prune(m.h, c.ctypes.data_as(C.POINTER(C.c_double)), 1.0, 64, C.byref(a), C.byref(b),
                                                  C.byref(k)) == CAPACITY
    assert (a.value, b.value, k.value) == (-7, -7, -7)


def _filled(twins, with_attr=True):
    m = twins(with_attr=with_attr)
    done, want = Rm.expected("prune:size-1025-alternate", "never", "all")
    Rm.replay(done[:2], want[:2], m)
    assert want[1][4] > 100
    return m, want[1]


def test_take_refusals_write_nothing_and_keep_the_log(twins):
    m, (_, rows, keys, words, n, _) = _filled(twins)
    L = capi.host_lib()
    k, x, w, got = np.full(n + 8, 0xAB, np.uint64), np.full((n + 8, 3), -3.5, np.float32), np.full(n + 8, 0xCD, np.uint32), C.c_int64(-7)
    canary = (k.tobytes(), x.tobytes(), w.tobytes())
    take = lambda kk, xx, ww, cap, nn: L.madicp_host_map_take_removed(  # noqa: E731
        m.h, None if kk is None else kk.ctypes.data_as(_u64p), None if xx is None else xx.ctypes.data_as(_fp),
        None if ww is None else ww.ctypes.data_as(_u32p), cap, None if nn is None else C.byref(nn))
    assert take(k, x, w, n - 1, got) == CAPACITY and got.value == n  # one short: the number needed, nothing written, the log kept
    assert (k.tobytes(), x.tobytes(), w.tobytes()) == canary and m.removed_count() == n
    got.value = -7
    for args in ((None, x, w, n, got), (k, None, w, n, got), (k, x, w, n, None)):
        assert take(*args) == INVALID
    assert capi.host_lib().madicp_host_map_take_removed(None, k.ctypes.data_as(_u64p), x.ctypes.data_as(_fp), None, n, C.byref(got)) == INVALID
    assert got.value == -7 and (k.tobytes(), x.tobytes(), w.tobytes()) == canary and m.removed_count() == n
    assert m.rows().tobytes() == rows.tobytes() and m.keys().tobytes() == keys.tobytes() and m.words().tobytes() == words.tobytes()
    assert take(k, x, None, n, got) == 0 and got.value == n and w.tobytes() == canary[2]  # (the words are optional)
    assert k[n:].tobytes() == canary[0][8 * n:] and m.removed_count() == 0
    plain, _ = _filled(twins, with_attr=False)  # out_attr on a map without the column
    assert L.madicp_host_map_take_removed(plain.h, k.ctypes.data_as(_u64p), x.ctypes.data_as(_fp), w.ctypes.data_as(_u32p), n + 8,
                                          C.byref(got)) == INVALID
    assert plain.removed_count() == n and w.tobytes() == canary[2]


def test_download_keys_and_rows(twins):
    """download_rows equals download_f32 + download_keys + download_attr at every window; the refusals write nothing"""
    m, (_, rows, keys, words, _, _) = _filled(twins)
    M = rows.shape[0]
    for first in (0, 1, M // 2, M - 1, M):
        x, k, w = capi.host_map_download_rows(m.h, first, True, True)
        assert x.tobytes() == capi.host_map_download_f32(m.h, first).tobytes() == rows[first:].tobytes()
        assert k.tobytes() == capi.host_map_download_keys(m.h, first).tobytes() == keys[first:].tobytes()
        assert w.tobytes() == capi.host_map_download_attr(m.h, first).tobytes() == words[first:].tobytes()
        assert capi.host_map_download_rows(m.h, first, False, False)[0].tobytes() == x.tobytes()
    L = capi.host_lib()
    k, x, w, got = np.full(M, 0xAB, np.uint64), np.full((M, 3), -3.5, np.float32), np.full(M, 0xCD, np.uint32), C.c_int64(-7)
    canary = (k.tobytes(), x.tobytes(), w.tobytes())
    kp, xp, wp = k.ctypes.data_as(_u64p), x.ctypes.data_as(_fp), w.ctypes.data_as(_u32p)
    assert L.madicp_host_map_download_keys(m.h, 0, kp, M - 1, C.byref(got)) == CAPACITY and got.value == M
    assert L.madicp_host_map_download_rows(m.h, 0, xp, kp, wp, M - 1, C.byref(got)) == CAPACITY and got.value == M
    got.value = -7
    for first in (-1, M + 1):
        assert L.madicp_host_map_download_keys(m.h, first, kp, M, C.byref(got)) == INVALID
        assert L.madicp_host_map_download_rows(m.h, first, xp, kp, wp, M, C.byref(got)) == INVALID
    assert L.madicp_host_map_download_keys(m.h, 0, None, M, C.byref(got)) == INVALID
    assert L.madicp_host_map_download_keys(m.h, 0, kp, M, None) == INVALID
    assert L.madicp_host_map_download_rows(m.h, 0, None, kp, wp, M, C.byref(got)) == INVALID
    assert L.madicp_host_map_download_rows(m.h, 0, xp, kp, wp, M, None) == INVALID
    plain, _ = _filled(twins, with_attr=False)
    assert L.madicp_host_map_download_rows(plain.h, 0, xp, kp, wp, M, C.byref(got)) == INVALID
    assert got.value == -7 and (k.tobytes(), x.tobytes(), w.tobytes()) == canary
    assert L.madicp_host_map_download_rows(m.h, M, xp, kp, wp, 0, C.byref(got)) == 0 and got.value == 0  # an empty window


def test_clear_empties_the_log(twins):
    steps = P.named("reentry")
    steps = steps[:2] + [("reset",)] + steps[2:] + [("take",)]
    done, want = Rm.run_ref(steps, watermark="all")
    assert want[1][4] > 0 and want[2][4] == 0 and want[-2][4] > 0
    Rm.replay(done, want, twins())
