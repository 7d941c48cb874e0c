"""Context.map_query (madicp_map_query_cloud: fe::map_query_lanes — fe::map_query_coop in a -DMADICP_QUERY_COOP build —
and fe::map_slot_rows on maps without the slot-to-row column) against the numpy restatement (tests/map_query_ref.py) and the host
twin, on plain, attribute, evidence and moments maps: cloud sizes around the kernel's geometry, voxel faces and the ends of the key range, which row wins, maps after growths,
a prune, a clearing and a wipe, a table whose probes wrap, 4 096 points in one voxel, the self-query, the scoring form, that the map
is only read, and every refusal.  Exact equality everywhere."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_query_ref as Q
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps and twin are fixtures)
from test_host_map_query import CAPACITY, INVALID, KINDS, SPECS, twin  # noqa: F401

pytestmark = pytest.mark.gpu


def everything(m):
    """every column the map has, as bytes"""
    return [c.tobytes() for c in (m.rows(), m.keys(), m.words(), m.evidence(), m.moments()) if c is not None]


@pytest.fixture
def made(ctx, maps, twin):
    """a device map of one of the four kinds (a scan gets its words on the kinds with the attribute column) and its host twin"""
    return (lambda kind="plain", **k: maps.dev(ctx, **{"voxel": Q.VOXEL, **SPECS[kind], **k})), twin


# (a resident cloud always holds a point — madicp_cloud_upload and the ingests refuse an empty one — so n = 0 is the host twin's case:
# tests/test_host_map_query.py)
@pytest.mark.parametrize("name", [s for s in Q.SIZE_NAMES if s != "size-0"] + Q.OTHER_NAMES)
def test_device_query_is_the_restatement_and_the_twin(made, name):
    dev, twin = made
    steps, asks = Q.named(name)
    cap = dict(max_rows=64) if name == "wrapping" else {}
    first = None
    for kind in KINDS:
        d, h = dev(kind, **cap), twin(kind, **cap)
        Q.build(d, steps)
        Q.build(h, steps)
        assert d.rows().tobytes() == h.rows().tobytes() and d.keys().tobytes() == h.keys().tobytes()
        want = Q.hold(d, asks, (name, kind, "device"))
        Q.hold(h, asks, (name, kind, "twin"))
        if first is None or not Q.same_rows_on_every_kind(steps):
            first = want
        for a, b in zip(first, want):  # the same row, d2 and key on all four kinds
            assert a["counts"] == b["counts"] and all(a[c].tobytes() == b[c].tobytes() for c in ("row", "d2", "keys")), (name, kind)
    if name == "wiped":
        assert all(w["counts"][1] == 0 and np.all(w["row"] == -1) for w in want)
    if name == "one_voxel":
        assert want[0]["counts"][:2] == (4096, 4096) and np.all(want[0]["row"] == 0)


def test_device_query_picks_the_winner(made):
    dev, _ = made
    for swap in (False, True):
        for kind in ("plain", "ev"):
            m = dev(kind)
            steps, asks = Q.winners(swap)
            Q.build(m, steps)
            cloud = asks[0][0]
            _, row1, d1 = m.query(cloud, *E.IDENTITY, 1, np.inf)
            counts0, row0, d0 = m.query(cloud, *E.IDENTITY, 0, np.inf)
            assert row1.tolist() == [1, 2, 3] and row0.tolist() == [0, -1, 3 if swap else 4] and counts0 == (3, 2, 2)
            assert d1[2] == 0.0625 and d0[2] == 0.0625 and np.isposinf(d0[1])


def test_device_self_query_finds_every_point(made):
    dev, _ = made
    R, t = E.random_pose(5)
    cloud = E.with_nonfinite(E.gaussian(3000, 8, scale=6.0), 2)
    cand, own = Q.cells_of(E.positions(cloud, R, t), Q.VOXEL)
    k = ((own[:, 0] + Q.HALF) | ((own[:, 1] + Q.HALF) << 21) | ((own[:, 2] + Q.HALF) << 42)).astype(np.uint64)
    for kind in KINDS:
        m = dev(kind)
        m.insert(cloud, R, t, None)
        (c, matched, within), row, d2, keys = m.query(cloud, R, t, 0, 2 * Q.VOXEL, True, True)
        assert c == matched == within == int(np.count_nonzero(cand)) and c < 3000
        assert np.array_equal(keys[cand], k[cand]) and np.all(keys[~cand] == Q.NO_KEY)


def test_device_query_only_reads(made):
    dev, _ = made
    steps, asks = Q.moved()
    more = E.gaussian(500, 99, scale=2.5)
    for kind in KINDS:
        a, b = dev(kind), dev(kind)
        Q.build(a, steps)
        Q.build(b, steps)
        before = everything(a)
        for cloud, R, t in asks:
            for reach in (0, 1):
                a.query(cloud, R, t, reach, 0.3, True, True)
                a.query(cloud, R, t, reach, 0.3, False)
        assert everything(a) == before == everything(b)
        assert a.insert(more, *E.IDENTITY, None) == b.insert(more, *E.IDENTITY, None)
        assert everything(a) == everything(b)
        assert a.clear_rays(asks[1][0], *E.IDENTITY, np.array([0.1, -0.2, 0.3])) == b.clear_rays(asks[1][0], *E.IDENTITY, np.array([0.1, -0.2, 0.3]))
        assert everything(a) == everything(b)


def _raw(ctx, mid, cid, R, t, reach, max_dist, bufs, capacity, counts, handle=True):
    p = lambda a, ct: None if a is None else a.ctypes.data_as(ct)
    dp = C.POINTER(C.c_double)
    types = (C.POINTER(C.c_int32), dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
    return capi.hip_lib().madicp_map_query_cloud(ctx._h if handle else None, mid, cid, p(R, dp), p(t, dp), reach, max_dist,
                                                 *[p(b, ct) for b, ct in zip(bufs, types)], capacity, p(counts, C.POINTER(C.c_uint64)))


def test_device_query_refusals_write_nothing(ctx, made):
    dev, _ = made
    plain, ev = dev("plain"), dev("ev")
    pts = np.ascontiguousarray(E.gaussian(40, 1))
    for m in (plain, ev):
        m.insert(pts, *E.IDENTITY, None)
    cid = ev.cloud(pts)
    R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
    bad_R, bad_t = R.copy(), t.copy()
    bad_R[4], bad_t[1] = np.nan, np.inf

    def fresh():
        return [np.full(40, -7, np.int32), np.full(40, -7.0), np.full(40, 7, np.uint64), np.full(40, 7, np.uint32), np.full(40, 7, np.uint32)], np.full(3, 7, np.uint64)

    def untouched(bufs, counts):
        return np.all(bufs[0] == -7) and np.all(bufs[1] == -7.0) and all(np.all(b == 7) for b in bufs[2:]) and np.all(counts == 7)

    def refused(code, mid, cloud, R_, t_, reach, max_dist, keep, capacity=40, with_counts=True, handle=True):
        bufs, counts = fresh()
        given = [b if k else None for b, k in zip(bufs, keep)]
        before = everything(ev) + everything(plain)
        assert _raw(ctx, mid, cloud, R_, t_, reach, max_dist, given, capacity, counts if with_counts else None, handle) == code
        assert untouched(bufs, counts) and everything(ev) + everything(plain) == before

    try:
        all5 = (1, 1, 1, 1, 1)
        refused(INVALID, ev.mid, cid, None, t, 1, 1.0, all5)
        refused(INVALID, ev.mid, cid, R, None, 1, 1.0, all5)
        refused(INVALID, ev.mid, cid, R, t, 1, 1.0, all5, with_counts=False)
        refused(INVALID, ev.mid, cid, R, t, 1, 1.0, all5, handle=False)
        refused(INVALID, 987654, cid, R, t, 1, 1.0, all5)
        refused(INVALID, ev.mid, 987654, R, t, 1, 1.0, all5)
        refused(INVALID, ev.mid, cid, bad_R, t, 1, 1.0, all5)
        refused(INVALID, ev.mid, cid, R, bad_t, 1, 1.0, all5)
        for reach in (-1, 2, 27):
            refused(INVALID, ev.mid, cid, R, t, reach, 1.0, all5)
        for max_dist in (np.nan, -1.0, -np.inf):
            refused(INVALID, ev.mid, cid, R, t, 1, max_dist, all5)
        refused(INVALID, plain.mid, cid, R, t, 1, 1.0, (1, 1, 1, 1, 0))  # out_attr on a map without the column
        refused(INVALID, plain.mid, cid, R, t, 1, 1.0, (1, 1, 1, 0, 1))  # out_ev on a map without the column
        for keep in (all5, (1, 0, 0, 0, 0), (0, 0, 0, 0, 1)):
            refused(CAPACITY, ev.mid, cid, R, t, 1, 1.0, keep, capacity=39)
        bufs, counts = fresh()
        assert _raw(ctx, ev.mid, cid, R, t, 1, np.inf, [None] * 5, 0, counts) == 0 and counts.tolist() == [40, 40, 40]  # the scoring form
    finally:
        ctx.cloud_release(cid)
