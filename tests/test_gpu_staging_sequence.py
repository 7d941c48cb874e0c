"""The pinned staging slot of the C ABI under ALL of its users on one long-lived context: cloud uploads on the float route and
on the plain route, tree uploads, both ingests and the stamped deskew, one after the other, at sizes that grow and shrink.

What one shared helper can get wrong and separate copies could not is the interplay: a slot handed out while its previous copy
is in flight, a grow between two users, a slot index tied to the wrong device landing block of the float route.  Every call of
the sequence is therefore held, byte for byte, to the same call made ALONE on a fresh context — each call's behaviour on its
own, which does not depend on the sequencing being right — and to its bit-equal host twin where there is one: the input itself
(uploads), madicp_host_ingest_records, madicp_host_deskew_stamped, the oracle's ingest.  No tolerance anywhere.

The sizes: 1 365 / 1 366 points are 4 095 / 4 098 values, either side of the float route's threshold of 4 096; 21 845 / 21 846 /
21 847 are 65 535 / 65 538 / 65 541 values around the 65 536 of one piece of the float route (one piece, then two); 70 000 makes
every slot grow after it has been used small; 1 is a tree without a top and a record block that ends in padding.  Six kinds of
call against seven sizes: the 42 steps meet every pair once, and because the deskew step stages twice (points, stamps) a kind
does not keep meeting the same one of the two slots."""
import contextlib
import functools

import numpy as np
import pytest

import deskew_stamped_ref as DR
import ingest_records_ref as R
import oracle_lib as O
from fixtures import B_MAX, B_MIN
from mad_icp_amd import capi

pytestmark = pytest.mark.gpu

HZ = DR.HZ
SIZES = (1365, 21846, 1, 70000, 1366, 21845, 21847)     # up, down, up, down ...
KINDS = ("upload_f32", "upload_f64", "tree", "ingest_f32", "ingest_records", "deskew_stamped")
STEPS = [(KINDS[i % len(KINDS)], SIZES[i % len(SIZES)]) for i in range(len(KINDS) * len(SIZES))]
LAYOUT = R.LAYOUTS["xyzirt22"]                           # 22-byte records: an odd count ends in two bytes of padding


def points(n, seed):
    rng = np.random.default_rng([seed, n])
    d = rng.normal(size=(n, 3))
    return np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2.0, 60.0, (n, 1)))


@functools.lru_cache(maxsize=None)
def inputs(kind, n):
    if kind == "upload_f32":
        return (points(n, 1).astype(np.float32).astype(np.float64),)
    if kind == "upload_f64":
        p = points(n, 2)
        assert (p[0].astype(np.float32).astype(np.float64) != p[0]).any()   # (found out in the first block: the plain route)
        return (p,)
    if kind == "tree":
        return (capi.HostTree(points(n, 3), B_MAX, B_MIN, 2),)
    if kind == "ingest_f32":
        xyz = R.patterned(R.survivors("alternating", n), n)
        return (np.ascontiguousarray(np.concatenate([xyz, np.ones((n, 1), np.float32)], axis=1)),)
    if kind == "ingest_records":
        return (R.pack(LAYOUT, R.patterned(R.survivors("alternating", n), n + 1), R.generic_times(LAYOUT, n, n), seed=n),)
    pts, stamps = points(n, 4), DR.mixed_stamps(n, seed=2)
    twin, v6, chunks = capi.host_deskew_stamped(pts, stamps, *DR.poses_for(DR.VELOCITIES["rodrigues"], HZ), HZ)
    return pts, stamps, v6, twin, chunks


def call(ctx, kind, n):
    """one call of the sequence and what it left on the device, as a dict of arrays"""
    args = inputs(kind, n)
    if kind == "tree":
        tid = ctx.upload(args[0])
        try:
            return {"nodes": ctx.tree_download(tid, args[0].num_nodes)}
        finally:
            ctx.tree_release(tid)
    if kind in ("upload_f32", "upload_f64"):
        cid, out = ctx.cloud_upload(args[0]), {}
    elif kind == "ingest_f32":
        cid, kept = ctx.cloud_ingest_f32(args[0], R.LO, R.HI, 1)
        out = {"kept": np.array([kept])}
    elif kind == "ingest_records":
        cid, kept, rng = ctx.cloud_ingest_records(args[0], R.LO, R.HI, 1, layout=LAYOUT)
        out = {"kept": np.array([kept]), "range": np.array(rng)}
    else:
        cid, out = ctx.cloud_upload(args[0]), {}
    try:
        if kind == "deskew_stamped":
            out["chunks"] = ctx.cloud_deskew_stamped(cid, args[1], args[2], HZ, want_chunks=True)
        if kind == "ingest_records":
            out["stamps"] = ctx.cloud_stamps(cid)
        out["xyz"] = ctx.cloud_download(cid)
    finally:
        ctx.cloud_release(cid)
    return out


def check_twin(kind, n, got):
    args = inputs(kind, n)
    if kind in ("upload_f32", "upload_f64"):
        assert got["xyz"].tobytes() == args[0].tobytes()
    elif kind == "tree":
        assert got["nodes"].tobytes() == args[0].nodes.tobytes()
    elif kind == "ingest_f32":
        assert R.same_bits(got["xyz"], O.ingest_f32(args[0][:, :3], R.LO, R.HI, 1))
    elif kind == "ingest_records":
        h_p, h_s, h_r = capi.host_ingest_records(args[0], R.LO, R.HI, 1, layout=LAYOUT)
        assert got["kept"][0] == h_p.shape[0] == (n + 1) // 2
        assert R.same_bits(got["xyz"], h_p) and R.same_bits(got["stamps"], h_s) and R.same_bits(got["range"], np.array(h_r))
    else:
        assert got["xyz"].view(np.uint64).tobytes() == args[3].view(np.uint64).tobytes()
        assert np.array_equal(got["chunks"], args[4])


def test_every_user_of_the_staging_slot_on_one_context(natives):
    assert sorted(set(STEPS)) == sorted((k, n) for k in KINDS for n in SIZES)                # every pair, once
    assert {1, 1365, 1366, 21846, 21847, 70000} <= set(SIZES)
    try:
        with contextlib.closing(capi.Context(0)) as shared:
            for step, (kind, n) in enumerate(STEPS):
                got = call(shared, kind, n)
                with contextlib.closing(capi.Context(0)) as fresh:
                    alone = call(fresh, kind, n)
                assert got.keys() == alone.keys()
                for name in got:
                    assert got[name].dtype == alone[name].dtype and got[name].shape == alone[name].shape, (step, kind, n, name)
                    assert got[name].tobytes() == alone[name].tobytes(), (step, kind, n, name)
                check_twin(kind, n, got)
    finally:
        inputs.cache_clear()                             # (the host trees go with it)
