"""The device map's evidence column (madicp_map_create_ev: fe::map_hit behind the claim, fe::map_clear_mark_ev in the clearing, the
column through fe::map_compact and map_grow; madicp_map_download_evidence / _download_min_evidence) against BOTH the numpy
restatement of tests/map_evidence_ref.py and the host twin, bit for bit after EVERY step: answers, rows, stored keys, words,
evidence, the log's count and what a take returns.  Clouds of 1, 63, 64, 65, 257 and 3 000 points; maps one row below, at and one
above the 1 024-mark scan tile and across two tiles; a table small enough that probes wrap past its last slot; a block grown from
one row, so that the slots' rows survive every growth and every rehash behind a removal; a fold directly behind a prune and behind
a clearing; 4 096 points in one voxel; 1/1/1 against a plain device map; every refusal."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_clear_ref as Cl
import map_evidence_ref as Ev
import map_removed_ref as Rm
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps and twins are fixtures)
from test_host_map_evidence import twins  # noqa: F401
from test_host_map_removed import CAPACITY, INVALID, TWIN

pytestmark = pytest.mark.gpu

_fp, _u64p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@pytest.fixture
def made(ctx, maps, twins):
    """device map / host twin factories; params None: a plain device map"""
    return (lambda params, **k: maps.dev(ctx, **{**TWIN, "voxel": Ev.VOXEL, "evidence": params, **k})), twins


@pytest.mark.parametrize("params", [(1, 1, 8), (3, 2, 7)])
@pytest.mark.parametrize("name", Ev.MIXED_NAMES)
def test_mixed_sequences(made, name, params):
    """clouds of 1 .. 3 000 points; a fold directly behind a clearing and directly behind a prune; a block grown from one row beside
    one created large, with and without the attribute column"""
    dev, twin = made
    done, want = Ev.expected(name, params)
    Ev.replay(done, want, dev(params, initial_rows=1), dev(params, initial_rows=1 << 13, with_attr=False), twin(params), tag=name,
              cap=params[2])


@pytest.mark.parametrize("name", Ev.ROW_NAMES)
def test_row_counts_around_the_scan_tile(made, name):
    dev, twin = made
    done, want = Ev.expected(name, (2, 3, 9))
    assert want[0][0][1] == int(name.split(":")[1])  # exactly that many rows under the marks
    Ev.replay(done, want, dev((2, 3, 9), initial_rows=1), twin((2, 3, 9)), tag=name, cap=9)


@pytest.mark.parametrize("name", ["growths", "prune_in_front", "old_and_new"])
def test_named_sequences(made, name):
    dev, twin = made
    done, want = Ev.expected(name, (1, 1, 4))
    Ev.replay(done, want, dev((1, 1, 4), initial_rows=1), dev((1, 1, 4), initial_rows=1 << 14, with_attr=False), twin((1, 1, 4)), tag=name,
              cap=4)
    assert sorted(set(want[-1][4].tolist())) != [1]


def test_4096_points_in_one_voxel_add_hit_once(made):
    dev, twin = made
    done, want = Ev.expected("one_voxel", (3, 1, 100))
    Ev.replay(done, want, dev((3, 1, 100)), dev((3, 1, 100), initial_rows=1), twin((3, 1, 100)), cap=100)
    assert [w[4].tolist() for w in want] == [[3, 3], [6, 3], [9, 3]]


def test_a_table_whose_probes_wrap(made):
    """cap = 64 rows, 128 slots, no growth: 32 keys that run past the last slot — claimed, found again by the fold's hits (the
    election is per SLOT), by the clearing's rays and rows, refilled behind the removal, and hit again"""
    dev, twin = made
    I, z = E.IDENTITY
    pts = Ev.wrapping_cloud(32, 128)
    rays = Cl.through(pts[::2], Cl.ORIGIN, np.full(16, 1.6))
    steps = [("fold", pts, I, z), ("fold", pts, I, z), ("clear", rays, I, z, Cl.ORIGIN, 0.0, 16), ("fold", pts[::-1], I, z),
             ("clear", rays, I, z, Cl.ORIGIN, 0.0, "all"), ("clear", rays, I, z, Cl.ORIGIN, 0.0, 0), ("fold", pts[:9], I, z)]
    done, want = Ev.run_ref(steps, (1, 1, 3))
    assert want[0][0] == (32, 32) and want[5][0][0] > 0  # every point a row; the third clearing does remove
    Ev.replay(done, want, dev((1, 1, 3), initial_rows=64, max_rows=64), twin((1, 1, 3), initial_rows=64, max_rows=64), cap=3)


def test_boundaries_saturation_and_decrements(made):
    dev, twin = made
    I, z = E.IDENTITY
    for params, steps in [((3, 3, 9), Ev.see_through(1)), ((4, 3, 9), Ev.see_through(2)), ((2, 2, 6), Ev.see_through(4, hits=3)),
                          ((3, 1, 10), [("fold", E.own_cells(5), I, z)] * 5),
                          ((Ev.CAP_MAX - 1, 1, Ev.CAP_MAX), [("fold", E.own_cells(5), I, z)] * 3)]:
        done, want = Ev.run_ref(steps, params)
        Ev.replay(done, want, dev(params, initial_rows=1), twin(params), tag=str(params), cap=params[2])


@pytest.mark.parametrize("name", ["prune:posed", "clear:size-1025-257", "clear:edges", "mixed:257"])
def test_one_one_one_is_the_plain_map(made, name):
    dev, _ = made
    steps = Rm.with_takes(Ev.named(name), "every")
    done, want = Ev.run_ref(steps, (1, 1, 1))
    Ev.replay(done, want, dev((1, 1, 1), initial_rows=1), dev(None, initial_rows=1), tag=name, cap=1)


def test_with_the_log_and_a_reset(made):
    dev, twin = made
    steps = Ev.mixed(257) + [("reset",)] + Ev.mixed(65)
    done, want = Ev.run_ref(Rm.with_takes(steps, "every"), (2, 1, 5))
    Ev.replay(done, want, dev((2, 1, 5), initial_rows=1), twin((2, 1, 5)), cap=5)


def test_refusals(ctx):
    L, h = capi.hip_lib(), ctx._h
    mid = C.c_int(-7)
    for hit, miss, cap in [(0, 1, 1), (1, 0, 1), (2, 1, 1), (1, 1, 2 ** 31), (2 ** 31, 1, 2 ** 32 - 1)]:
        assert L.madicp_map_create_ev(h, 0.5, 1, 100, 0, hit, miss, cap, C.byref(mid)) == INVALID and mid.value == -7
    assert L.madicp_map_create_ev(h, 0.0, 1, 100, 0, 1, 1, 1, C.byref(mid)) == INVALID
    assert L.madicp_map_create_ev(h, 0.5, 1, 100, 0, 1, 1, 1, None) == INVALID
    I, z = E.IDENTITY
    n = C.c_int64(-7)
    xyz, ev, keys = np.full((8, 3), 7.0, np.float32), np.full(8, 77, np.uint32), np.full(8, 77, np.uint64)
    cid6, cid3 = ctx.cloud_upload(E.own_cells(6)), ctx.cloud_upload(E.own_cells(3))
    for make in (ctx.map_create, ctx.map_create_attr):  # the downloads on a plain map
        p = make(0.5, 1, 100)
        ctx.map_insert_cloud(p, cid6, I, z)
        assert L.madicp_map_download_evidence(h, p, 0, ev.ctypes.data_as(_u32p), 8, C.byref(n)) == INVALID
        assert L.madicp_map_download_min_evidence(h, p, 0, xyz.ctypes.data_as(_fp), None, None, None, 8, C.byref(n)) == INVALID
        assert n.value == -7 and np.all(ev == 77) and np.all(xyz == 7.0)
        ctx.map_release(p)
    m = ctx.map_create_ev(0.5, 1, 100, 2, 1, 4)
    ctx.map_insert_cloud(m, cid6, I, z)
    ctx.map_insert_cloud(m, cid3, I, z)
    assert L.madicp_map_download_evidence(h, m, 1, ev.ctypes.data_as(_u32p), 4, C.byref(n)) == CAPACITY and n.value == 5
    assert L.madicp_map_download_min_evidence(h, m, 3, xyz.ctypes.data_as(_fp), keys.ctypes.data_as(_u64p), None, ev.ctypes.data_as(_u32p), 2,
                                              C.byref(n)) == CAPACITY and n.value == 3
    assert np.all(ev == 77) and np.all(xyz == 7.0) and np.all(keys == 77)
    assert L.madicp_map_download_min_evidence(h, m, 3, xyz.ctypes.data_as(_fp), None, None, ev.ctypes.data_as(_u32p), 3, C.byref(n)) == 0
    assert n.value == 3 and ev[:3].tolist() == [4, 4, 4] and ev[3] == 77
    assert L.madicp_map_download_min_evidence(h, m, 5, xyz.ctypes.data_as(_fp), None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert L.madicp_map_download_evidence(h, m, 7, ev.ctypes.data_as(_u32p), 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_evidence(h, m, 0, None, 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_evidence(h, m, 0, ev.ctypes.data_as(_u32p), 8, None) == INVALID
    assert L.madicp_map_download_min_evidence(h, m, 0, None, None, None, None, 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_min_evidence(h, m, 0, xyz.ctypes.data_as(_fp), None, ev.ctypes.data_as(_u32p), None, 8, C.byref(n)) == INVALID
    assert L.madicp_map_download_evidence(h, m + 1000, 0, ev.ctypes.data_as(_u32p), 8, C.byref(n)) == INVALID
    assert ctx.map_download_evidence(m).tolist() == [4, 4, 4, 2, 2, 2]  # ... and nothing of it changed the map
    ctx.map_clear(m)
    assert L.madicp_map_download_min_evidence(h, m, 0, xyz.ctypes.data_as(_fp), None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    ctx.map_insert_cloud(m, cid3, I, z)  # cleared: the words are forgotten with the rows
    assert ctx.map_download_evidence(m).tolist() == [2, 2, 2]
    ctx.map_release(m)
    ctx.cloud_release(cid6)
    ctx.cloud_release(cid3)
