"""The device map's removal log (madicp_map_track_removed / _removed_count / _take_removed: fe::map_log_removed beside fe::map_compact,
behind the scan that map_remove_marked already has) and its key and row downloads (madicp_map_download_keys / _download_rows)
against BOTH the numpy restatement of tests/map_removed_ref.py and the host twin, bit for bit after EVERY step of the sequences of
tests/map_prune_ref.py and tests/map_clear_ref.py: answers, rows, stored keys, words, the log's count and what a take returns.
Map sizes over the wavefront, the workgroup and the 1 024-mark scan tile; taking after every step and only at the end (a base
behind entries already there, the log's growth); the watermarks 0, 1, M/2, M - 1 and M; one row logged, then 4 097; re-entry; with
and without the column; tracking off, switched on and off; the full log; every refusal; two maps; a map far larger than any cloud
its context has seen; a block grown from one row; the log across a growth of the map."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloud_export_ref as E
import map_prune_ref as P
import map_removed_ref as Rm
from mad_icp_amd import capi
from map_impls import DevImpl, maps  # noqa: F401 (maps is a fixture)
from test_host_map_removed import (CAPACITY, CLEAR_NAMES, INVALID, PRUNE_NAMES, WATERMARK_NAMES, TWIN, logged, one_then_4097)

pytestmark = pytest.mark.gpu

_fp, _u64p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@pytest.fixture
def made(ctx, maps):
    """device map / host twin factories"""
    return functools.partial(maps.dev, ctx, **TWIN), functools.partial(maps.host, **TWIN)


@pytest.mark.parametrize("cadence", ["every", "end"])
@pytest.mark.parametrize("name", PRUNE_NAMES + CLEAR_NAMES)
def test_sequences(made, name, cadence):
    dev, twin = made
    done, want = Rm.expected(name, cadence)
    Rm.replay(done, want, dev(), twin(), tag=name)


@pytest.mark.parametrize("watermark", Rm.WATERMARKS[1:])
@pytest.mark.parametrize("name", WATERMARK_NAMES)
def test_watermarks(made, name, watermark):
    dev, twin = made
    done, want = Rm.expected(name, "every", watermark)
    Rm.replay(done, want, dev(), dev(with_attr=False), twin(), tag=name)


@pytest.mark.parametrize("name", ["prune:posed", "prune:growth", "clear:size-4097-257", "clear:everything"])
def test_initial_rows_1_and_accumulated_takes(made, name):
    """a block grown from one row against a map created large, no column against the column, one take at the end: the removals pile
    up behind a base, the log grows, and it survives the growths of the map behind a removal"""
    dev, _ = made
    done, want = Rm.expected(name, "end")
    assert logged(want) > 0
    Rm.replay(done, want, dev(initial_rows=1), dev(initial_rows=1 << 15), dev(initial_rows=1, with_attr=False), tag=name)


def test_one_row_then_4097(made):
    dev, twin = made
    done, want = Rm.run_ref(one_then_4097())
    Rm.replay(done, want, dev(initial_rows=1), dev(with_attr=False), twin())


def test_reentry_logs_a_key_twice(made):
    dev, twin = made
    done, want = Rm.expected("prune:reentry", "every", "all")
    Rm.replay(done, want, dev(), twin(), tag="reentry")


@pytest.mark.parametrize("name", PRUNE_NAMES + CLEAR_NAMES)
def test_tracking_off_changes_nothing(made, name):
    dev, _ = made
    off_done, off = Rm.expected(name, "never", tracking=False)
    on_done, on = Rm.expected(name, "never")
    Rm.replay(off_done, off, dev(tracking=False), tag=name)
    Rm.replay(on_done, on, dev(), tag=name)


def test_tracking_switched_mid_sequence(made):
    dev, twin = made
    steps = P.named("posed")
    steps = steps[:2] + [("track", True)] + steps[2:4] + [("track", False)] + steps[4:] + [("track", True), ("take",)]
    done, want = Rm.run_ref(steps, tracking=False)
    Rm.replay(done, want, dev(initial_rows=1, tracking=False), twin(tracking=False))


def test_the_log_is_bounded_by_max_rows(made):
    dev, twin = made
    I, z = E.IDENTITY
    cells, far = E.own_cells(64), np.array([1.0e4, 0.0, 0.0])
    steps = [("fold", cells, I, z), ("prune", far, 1.0, "all"), ("fold", cells, I, z), ("prune", far, 1.0, "all"),
             ("clear", cells * 1.5, I, z, np.zeros(3), 0.0, "all"), ("take",), ("prune", far, 1.0, "all"), ("take",)]
    done, want = Rm.run_ref(steps, max_rows=64)
    assert [w[0] for w in want] == [(64, 64), (64, 0, 0), (64, 64), None, None, None, (64, 0, 0), None]
    Rm.replay(done, want, dev(initial_rows=64, max_rows=64), dev(initial_rows=1, max_rows=64, with_attr=False),
              twin(initial_rows=64, max_rows=64))


def test_two_maps_interleaved(made):
    """two tracking maps of one context, one step each in turn: each log is its own"""
    dev, _ = made
    a, b = dev(initial_rows=1), dev(with_attr=False)
    (da, wa), (db, wb) = Rm.expected("prune:posed", "end"), Rm.expected("clear:size-1025-257", "end")
    for i in range(max(len(da), len(db))):
        if i < len(da):
            Rm.replay(da[i:i + 1], wa[i:i + 1], a, tag="a%d" % i)
        if i < len(db):
            Rm.replay(db[i:i + 1], wb[i:i + 1], b, tag="b%d" % i)
    assert logged(wa) > 0 and logged(wb) > 0


def test_a_map_larger_than_any_cloud_its_context_has_seen(natives):
    """map_prune_ref.large's 20 480-row map in a context that has seen only 256-point clouds: the log's kernel is sized by the map"""
    c = capi.Context(0)
    try:
        m = DevImpl(c, initial_rows=1, **TWIN)
        done, want = Rm.expected("prune:large", "end", "all")
        assert logged(want) > 5000
        Rm.replay(done, want, m, tag="large")
        m.close()
    finally:
        c.close()


def _filled(dev, with_attr=True):
    m = dev(with_attr=with_attr)
    done, want = Rm.expected("prune:size-1025-alternate", "never", "all")
    Rm.replay(done[:2], want[:2], m)
    return m, want[1]


def test_take_refusals_write_nothing_and_keep_the_log(made, ctx):
    dev, _ = made
    m, (_, rows, keys, words, n, _) = _filled(dev)
    L, h = capi.hip_lib(), ctx._h
    k, x, w, got = np.full(n + 8, 0xAB, np.uint64), np.full((n + 8, 3), -3.5, np.float32), np.full(n + 8, 0xCD, np.uint32), C.c_int64(-7)
    canary = (k.tobytes(), x.tobytes(), w.tobytes())
    kp, xp, wp = k.ctypes.data_as(_u64p), x.ctypes.data_as(_fp), w.ctypes.data_as(_u32p)
    assert L.madicp_map_take_removed(h, m.mid, kp, xp, wp, n - 1, C.byref(got)) == CAPACITY and got.value == n
    assert (k.tobytes(), x.tobytes(), w.tobytes()) == canary and m.removed_count() == n
    got.value = -7
    assert L.madicp_map_take_removed(h, m.mid, None, xp, wp, n, C.byref(got)) == INVALID
    assert L.madicp_map_take_removed(h, m.mid, kp, None, wp, n, C.byref(got)) == INVALID
    assert L.madicp_map_take_removed(h, m.mid, kp, xp, wp, n, None) == INVALID
    assert L.madicp_map_take_removed(None, m.mid, kp, xp, wp, n, C.byref(got)) == INVALID
    assert L.madicp_map_take_removed(h, m.mid + 1000, kp, xp, wp, n, C.byref(got)) == INVALID
    assert L.madicp_map_removed_count(h, m.mid + 1000, C.byref(got)) == INVALID and L.madicp_map_removed_count(h, m.mid, None) == INVALID
    assert L.madicp_map_track_removed(h, m.mid + 1000, 1) == INVALID
    off = dev(tracking=False)
    assert L.madicp_map_take_removed(h, off.mid, kp, xp, None, n, C.byref(got)) == INVALID  # a map that does not track
    plain, _ = _filled(dev, with_attr=False)  # out_attr on a map without the column
    assert L.madicp_map_take_removed(h, plain.mid, kp, xp, wp, n + 8, C.byref(got)) == INVALID
    assert got.value == -7 and (k.tobytes(), x.tobytes(), w.tobytes()) == canary and m.removed_count() == plain.removed_count() == n
    assert m.rows().tobytes() == rows.tobytes() and m.keys().tobytes() == keys.tobytes() and m.words().tobytes() == words.tobytes()
    assert L.madicp_map_take_removed(h, m.mid, kp, xp, None, n, C.byref(got)) == 0 and got.value == n  # (the words are optional)
    assert w.tobytes() == canary[2] and k[n:].tobytes() == canary[0][8 * n:] and m.removed_count() == 0


def test_download_rows_is_the_three_downloads(made, ctx):
    """download_rows equals download_f32 + download_keys + download_attr, byte for byte, at every window; refusals write nothing"""
    dev, _ = made
    m, (_, rows, keys, words, _, _) = _filled(dev)
    M = rows.shape[0]
    for first in (0, 1, M // 2, M - 1, M):
        x, k, w = ctx.map_download_rows(m.mid, first, True, True)
        assert x.tobytes() == ctx.map_download_f32(m.mid, first).tobytes() == rows[first:].tobytes()
        assert k.tobytes() == ctx.map_download_keys(m.mid, first).tobytes() == keys[first:].tobytes()
        assert w.tobytes() == ctx.map_download_attr(m.mid, first).tobytes() == words[first:].tobytes()
        assert ctx.map_download_rows(m.mid, first, False, False)[0].tobytes() == x.tobytes()
    L, h = capi.hip_lib(), ctx._h
    k, x, w, got = np.full(M, 0xAB, np.uint64), np.full((M, 3), -3.5, np.float32), np.full(M, 0xCD, np.uint32), C.c_int64(-7)
    canary = (k.tobytes(), x.tobytes(), w.tobytes())
    kp, xp, wp = k.ctypes.data_as(_u64p), x.ctypes.data_as(_fp), w.ctypes.data_as(_u32p)
    assert L.madicp_map_download_keys(h, m.mid, 0, kp, M - 1, C.byref(got)) == CAPACITY and got.value == M
    assert L.madicp_map_download_rows(h, m.mid, 0, xp, kp, wp, M - 1, C.byref(got)) == CAPACITY and got.value == M
    got.value = -7
    for first in (-1, M + 1):
        assert L.madicp_map_download_keys(h, m.mid, first, kp, M, C.byref(got)) == INVALID
        assert L.madicp_map_download_rows(h, m.mid, first, xp, kp, wp, M, C.byref(got)) == INVALID
    assert L.madicp_map_download_keys(h, m.mid, 0, None, M, C.byref(got)) == INVALID
    assert L.madicp_map_download_keys(h, m.mid, 0, kp, M, None) == INVALID
    assert L.madicp_map_download_keys(h, m.mid + 1000, 0, kp, M, C.byref(got)) == INVALID
    assert L.madicp_map_download_rows(h, m.mid, 0, None, kp, wp, M, C.byref(got)) == INVALID
    assert L.madicp_map_download_rows(h, m.mid, 0, xp, kp, wp, M, None) == INVALID
    assert L.madicp_map_download_rows(h, m.mid + 1000, 0, xp, kp, wp, M, C.byref(got)) == INVALID
    plain, _ = _filled(dev, with_attr=False)
    assert L.madicp_map_download_rows(h, plain.mid, 0, xp, kp, wp, M, C.byref(got)) == INVALID
    assert got.value == -7 and (k.tobytes(), x.tobytes(), w.tobytes()) == canary
    assert L.madicp_map_download_rows(h, m.mid, M, xp, kp, wp, 0, C.byref(got)) == 0 and got.value == 0  # an empty window


def test_a_refused_removal_writes_nothing(made, ctx):
    dev, _ = made
    m = dev(initial_rows=64, max_rows=64)
    I, z = E.IDENTITY
    cells, far = E.own_cells(64), np.ascontiguousarray(np.array([1.0e4, 0.0, 0.0]))
    assert m.insert(cells, I, z, None) == (64, 64) and m.prune(far, 1.0, 64) == (64, 0, 0) and m.insert(cells, I, z, None) == (64, 64)
    before = (m.rows().tobytes(), m.keys().tobytes(), m.words().tobytes())
    a, b, k = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    assert capi.hip_lib().madicp_map_prune(ctx._h, m.mid, far.ctypes.data_as(C.POINTER(C.c_double)), 1.0, 64, C.byref(a), C.byref(b),
                                           C.byref(k)) == CAPACITY
    assert (a.value, b.value, k.value) == (-7, -7, -7) and m.removed_count() == 64
    assert (m.rows().tobytes(), m.keys().tobytes(), m.words().tobytes()) == before


def test_clear_empties_the_log(made):
    dev, twin = made
    steps = P.named("reentry")
    steps = steps[:2] + [("reset",)] + steps[2:] + [("take",)]
    done, want = Rm.run_ref(steps, watermark="all")
    Rm.replay(done, want, dev(), twin())
