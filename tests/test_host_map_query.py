"""The host twin's map query (madicp_host_map_query, csrc/host/voxel_map.h: VoxelMap::query) against the numpy restatement
(tests/map_query_ref.py) on every shared scenario, on plain, attribute, evidence and moments maps — exact equality everywhere — and
the restatement's sorted search against its own brute force.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_query_ref as Q
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)

INVALID, CAPACITY = -1, -4
KINDS = ["plain", "attr", "ev", "mom"]


# the four kinds of map this suite and tests/test_gpu_map_query.py query, as what the adapters of tests/map_impls.py take
SPECS = {"plain": dict(), "attr": dict(with_attr=True), "ev": dict(with_attr=True, evidence=(2, 1, 6)), "mom": dict(max_count=4)}


@pytest.fixture
def twin(maps):
    """a host map of one of the four kinds; its folds always go through madicp_host_map_insert_attr"""
    return lambda kind="plain", **k: maps.host(**{"voxel": Q.VOXEL, "insert_attr": True, **SPECS[kind], **k})


@pytest.mark.parametrize("name", Q.SIZE_NAMES + Q.OTHER_NAMES)
def test_host_query_is_the_restatement(twin, name):
    steps, asks = Q.named(name)
    first = None
    for kind in KINDS:
        m = twin(kind, max_rows=64 if name == "wrapping" else 1 << 24)
        Q.build(m, steps)
        want = Q.hold(m, asks, (name, kind))
        if first is None or not Q.same_rows_on_every_kind(steps):
            first = want
        for a, b in zip(first, want):  # the same row, d2 and key on all four kinds
            assert a["counts"] == b["counts"] and all(a[c].tobytes() == b[c].tobytes() for c in ("row", "d2", "keys")), (name, kind)


@pytest.mark.parametrize("name", ["size-257", "faces", "winners", "moved", "wrapping"])
def test_restatement_is_its_own_brute_force(twin, name):
    steps, asks = Q.named(name)
    m = twin("ev")
    Q.build(m, steps)
    for cloud, R, t in asks:
        for reach in (0, 1):
            a = Q.query(m.rows(), m.keys(), cloud, R, t, Q.VOXEL, reach, 0.3, m.words(), m.evidence())
            b = Q.query_brute(m.rows(), m.keys(), cloud, R, t, Q.VOXEL, reach, 0.3, m.words(), m.evidence())
            assert a["counts"] == b["counts"] and all(a[c].tobytes() == b[c].tobytes() for c in Q.COLUMNS), (name, reach)


def test_host_query_edges_say_what_they_should(twin):
    m = twin("plain")
    steps, asks = Q.faces()
    Q.build(m, steps)
    e = E.CELL * Q.VOXEL
    ask = np.array([[np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0], [e, 0.0, 0.0], [np.nextafter(e, 0.0)] * 3, [-e] * 3, [-1e-20, 0.25, 0.25]])
    (cand, matched, within), row, d2, keys = m.query(ask, *E.IDENTITY, 1, np.inf, True, True)
    assert (cand, matched, within) == (3, 3, 3)
    assert row[:3].tolist() == [-1, -1, -1] and np.all(np.isposinf(d2[:3])) and np.all(keys[:3] == Q.NO_KEY)
    top = (1 << 21) - 1
    assert int(keys[3]) == top | top << 21 | top << 42 and int(keys[4]) == 0 and d2[4] == 0.0
    assert int(keys[5]) == ((1 << 20) - 1) | (1 << 20) << 21 | (1 << 20) << 42  # (-1e-20 lies in cell -1)


def test_host_query_picks_the_winner(twin):
    for swap in (False, True):
        m = twin("plain")
        steps, asks = Q.winners(swap)
        Q.build(m, steps)
        cloud = asks[0][0]
        _, row1, d1 = m.query(cloud, *E.IDENTITY, 1, np.inf)
        counts0, row0, d0 = m.query(cloud, *E.IDENTITY, 0, np.inf)
        assert row1.tolist() == [1, 2, 3] and row0.tolist() == [0, -1, 3 if swap else 4] and counts0 == (3, 2, 2)
        assert d1[2] == 0.0625 and d0[2] == 0.0625 and np.isposinf(d0[1])


def test_host_self_query_finds_every_point(twin):
    for kind in KINDS:
        m = twin(kind)
        R, t = E.random_pose(5)
        cloud = E.with_nonfinite(E.gaussian(3000, 8, scale=6.0), 2)
        m.insert(cloud, R, t, None)
        cand, own = Q.cells_of(E.positions(cloud, R, t), Q.VOXEL)
        (c, matched, within), row, d2, keys = m.query(cloud, R, t, 0, 2 * Q.VOXEL, True, True)
        assert c == matched == within == int(np.count_nonzero(cand)) and c < 3000
        k = (own[:, 0] + Q.HALF) | ((own[:, 1] + Q.HALF) << 21) | ((own[:, 2] + Q.HALF) << 42)
        assert np.array_equal(keys[cand], k[cand].astype(np.uint64)) and np.all(keys[~cand] == Q.NO_KEY)


def test_host_query_only_reads(twin):
    for kind in KINDS:
        a, b = twin(kind), twin(kind)
        steps, asks = Q.moved()
        Q.build(a, steps)
        Q.build(b, steps)
        for cloud, R, t in asks:
            a.query(cloud, R, t, 1, 0.3, True, True)
        more = E.gaussian(500, 99, scale=2.5)
        assert a.insert(more, *E.IDENTITY, None) == b.insert(more, *E.IDENTITY, None)
        assert a.rows().tobytes() == b.rows().tobytes() and a.keys().tobytes() == b.keys().tobytes()
        if kind == "ev":
            assert a.evidence().tobytes() == b.evidence().tobytes() and a.words().tobytes() == b.words().tobytes()
        if kind == "mom":
            assert capi.host_map_download_moments(a.h).tobytes() == capi.host_map_download_moments(b.h).tobytes()


def _raw(h, cloud, R, t, reach, max_dist, bufs, capacity, counts, n=None):
    p = lambda a, ct: None if a is None else a.ctypes.data_as(ct)
    dp, L = C.POINTER(C.c_double), capi.host_lib()
    types = (C.POINTER(C.c_int32), dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
    return L.madicp_host_map_query(h, p(cloud, dp), cloud.shape[0] if n is None else n, p(R, dp), p(t, dp), reach, max_dist,
                                   *[p(b, ct) for b, ct in zip(bufs, types)], capacity, p(counts, C.POINTER(C.c_uint64)))


def test_host_query_refusals_write_nothing(twin):
    plain, ev = twin("plain"), twin("ev")
    cloud = np.ascontiguousarray(E.gaussian(40, 1))
    for m in (plain, ev):
        m.insert(cloud, *E.IDENTITY, None)
    R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
    bad_R, bad_t = R.copy(), t.copy()
    bad_R[4], bad_t[1] = np.nan, np.inf

    def fresh():
        return [np.full(40, -7, np.int32), np.full(40, -7.0), np.full(40, 7, np.uint64), np.full(40, 7, np.uint32), np.full(40, 7, np.uint32)], np.full(3, 7, np.uint64)

    def untouched(bufs, counts):
        return (np.all(bufs[0] == -7) and np.all(bufs[1] == -7.0) and all(np.all(b == 7) for b in bufs[2:]) and np.all(counts == 7))

    def refused(code, h, R_, t_, reach, max_dist, keep, capacity=40, with_counts=True):
        bufs, counts = fresh()
        given = [b if k else None for b, k in zip(bufs, keep)]
        assert _raw(h, cloud, R_, t_, reach, max_dist, given, capacity, counts if with_counts else None) == code
        assert untouched(bufs, counts)

    all5, no_ev, no_words = (1, 1, 1, 1, 1), (1, 1, 1, 1, 0), (1, 1, 1, 0, 0)
    refused(INVALID, ev.h, None, t, 1, 1.0, all5)
    refused(INVALID, ev.h, R, None, 1, 1.0, all5)
    refused(INVALID, ev.h, R, t, 1, 1.0, all5, with_counts=False)
    refused(INVALID, None, R, t, 1, 1.0, all5)
    refused(INVALID, ev.h, bad_R, t, 1, 1.0, all5)
    refused(INVALID, ev.h, R, bad_t, 1, 1.0, all5)
    for reach in (-1, 2, 27):
        refused(INVALID, ev.h, R, t, reach, 1.0, all5)
    for max_dist in (np.nan, -1.0, -np.inf):
        refused(INVALID, ev.h, R, t, 1, max_dist, all5)
    refused(INVALID, plain.h, R, t, 1, 1.0, no_ev)      # out_attr on a map without the column
    refused(INVALID, plain.h, R, t, 1, 1.0, (1, 1, 1, 0, 1))  # out_ev on a map without the column
    for keep in (all5, (1, 0, 0, 0, 0), (0, 0, 0, 0, 1)):
        refused(CAPACITY, ev.h, R, t, 1, 1.0, keep, capacity=39)
    bufs, counts = fresh()
    assert _raw(ev.h, cloud, R, t, 1, np.inf, [None] * 5, 0, counts) == 0 and counts.tolist() == [40, 40, 40]  # the scoring form needs no capacity
    bufs, counts = fresh()
    assert _raw(plain.h, None, R, t, 1, 0.0, [b if k else None for b, k in zip(bufs, no_words)], 0, counts, n=0) == 0
    assert counts.tolist() == [0, 0, 0] and untouched(bufs, np.full(3, 7, np.uint64))
