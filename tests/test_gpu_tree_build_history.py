"""The device tree build is the FRESH build, whatever the context built before.

The builder (mad_icp_amd/csrc/hip/tree_build.hip.h, driven by tree_build_begin_on / tree_build_end_on in frontend_capi.inc.h)
is documented as a function of (cloud, b_max, b_min).  Its launch schedule is not: a context remembers the point count, depth,
leaf count and work per step of its last build, and behind a cloud of similar size the next build launches fewer steps, crops
their grids, and emits into a block sized before the host knows the leaf count.  Consecutive scans of one sensor make every
hint right; here every pair of builds is chosen to make one hint WRONG (tests/tree_history_clouds.py; that it is wrong is held
on the CPU by tests/test_tree_history_clouds.py), and the tree must not change by a bit:

  * the reference of a cloud is its build as the FIRST build of a context of its own, held to the host builder by the criteria
    of tests/test_gpu_frontend.py (`right` links, leaf count, >= 99.9 % leaf representatives bitwise, valid preorder, every leaf
    mean its own nearest neighbour at distance 0) and cached as bytes;
  * every build under a history gives those bytes and the same (n_nodes, n_leaves);
  * what tree_download does not show — screening records, leaf records, the LDS-staged top, all written by tb_emit, in the
    pre-sized form from device-side counts — is held through its readers for every such tree of >= 1 000 leaves: nn_search of
    16 384 queries with and without the staged top against the numpy descent, and streamed registrations with the tree as the
    moving and as the fixed side against the same calls on the uploaded reference bytes.

Every comparison is an equality."""
import zlib

import numpy as np
import pytest

import tree_history_clouds as Cl
from descent_ref import descend
from fixtures import PARAMS
from mad_icp_amd import capi
from test_gpu_frontend import build_both, check_exact_properties

pytestmark = pytest.mark.gpu

N_QUERIES = 16384        # (nn_search stages the top from 16 k queries on: option "nn_lds_top")
RECORDS_MIN_LEAVES = 1000
ROUNDS = 4
T0 = np.eye(4)
T0[:3, :3] = [[np.cos(0.02), -np.sin(0.02), 0.0], [np.sin(0.02), np.cos(0.02), 0.0], [0.0, 0.0, 1.0]]
T0[:3, 3] = [0.3, -0.2, 0.05]

_FRESH = {}  # cloud name -> what its build on a context of its own gave


def queries(cloud):
    rng = np.random.default_rng(zlib.crc32(cloud.name.encode()))
    return cloud.pts[np.arange(N_QUERIES) % cloud.pts.shape[0]] + rng.normal(size=(N_QUERIES, 3)) * 0.05


def fresh(cloud):
    """The tree of `cloud` as the first build of a context that has built nothing, held to the host builder."""
    e = _FRESH.get(cloud.name)
    if e is not None:
        return e
    ctx = capi.Context(0)
    try:
        ht, cid, tid, nodes = build_both(ctx, cloud.pts, cloud.b_max, cloud.b_min)
        e = dict(nodes=nodes, info=ctx.tree_info(tid), depth=ctx.tree_build_stats()["max_level"])
        hn = ht.nodes
        assert e["info"] == (hn.shape[0], ht.num_leaves), (cloud.name, e["info"], hn.shape[0])
        assert np.array_equal(nodes["right"], hn["right"]), cloud.name
        assert e["depth"] == Cl.depth(hn)
        leaf = nodes["right"] == 0
        same = np.all(nodes["mean"][leaf].view(np.uint64) == hn["mean"][leaf].view(np.uint64), axis=1)
        assert same.mean() >= 0.999, (cloud.name, same.mean(), int((~same).sum()))
        check_exact_properties(ctx, cloud.pts, tid, nodes)
        if ht.num_leaves >= RECORDS_MIN_LEAVES:
            q = queries(cloud)
            r = ctx.nn_search(tid, q, want=("leaf", "dist"))
            e["leaf"] = descend(nodes, q)["leaf"]
            e["dist"] = r["dist"]
            assert np.array_equal(r["leaf"], e["leaf"]), cloud.name
        ctx.tree_release(tid)
        ctx.cloud_release(cid)
    finally:
        ctx.close()
    _FRESH[cloud.name] = e
    return e


def same_bits(a, b, what):
    for k in ("X", "H", "b", "matched"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert a["n_matched"] == b["n_matched"], what


class History:
    """Builds on ONE context, each held to the fresh build of its cloud."""

    def __init__(self, ctx, scenario):
        self.ctx, self.scenario, self.last, self.pairs = ctx, scenario, "-", 0
        self._fixed, self._ref = {}, {}

    def build(self, cloud, via):
        """-> (tree id, leaves); raises what the library raises (nothing is left behind then)"""
        ctx = self.ctx
        if via == "lookahead":
            ctx.tree_build_begin(cloud.pts, cloud.b_max, cloud.b_min)
            return ctx.tree_build_end()
        cid = ctx.cloud_upload(cloud.pts)
        try:
            return ctx.tree_build(cid, cloud.b_max, cloud.b_min)
        finally:
            ctx.cloud_release(cid)

    def held(self, cloud, via, records=True, keep=False):
        """Builds `cloud` behind whatever was built last and holds it to its fresh build."""
        f = fresh(cloud)
        ctx = self.ctx
        tid, nl = self.build(cloud, via)
        depth = ctx.tree_build_stats()["max_level"]
        info = ctx.tree_info(tid)
        print("scenario %s [%s] %s -> %s: depth %d, %d leaves" % (self.scenario, via, self.last, cloud.name, depth, info[1]))
        what = (self.scenario, via, self.last, cloud.name)
        self.last, self.pairs = cloud.name, self.pairs + 1
        assert (info, nl, depth) == (f["info"], f["info"][1], f["depth"]), what
        assert ctx.tree_download(tid, info[0]).tobytes() == f["nodes"].tobytes(), what
        if records and nl >= RECORDS_MIN_LEAVES:
            self.records(cloud, tid, f, what)
        if keep:
            return tid
        ctx.tree_release(tid)

    def fixed(self, cloud):
        """the reference bytes of `cloud` as a resident tree of this context (validating upload)"""
        if cloud.name not in self._fixed:
            f = fresh(cloud)
            self._fixed[cloud.name] = self.ctx.tree_upload(f["nodes"], f["info"][1])
        return self._fixed[cloud.name]

    def register(self, moving, fixed, nl):
        return self.ctx.stream_collect(self.ctx.stream_submit_tree(moving, [fixed], T0, PARAMS, ROUNDS), nl)

    def records(self, cloud, tid, f, what):
        ctx = self.ctx
        q = queries(cloud)
        before = ctx.get_option("nn_lds_top")
        try:
            for top in (0, 1):
                ctx.set_option("nn_lds_top", top)
                r = ctx.nn_search(tid, q, want=("leaf", "dist"))
                assert np.array_equal(r["leaf"], f["leaf"]), (what, top)
                assert r["dist"].tobytes() == f["dist"].tobytes(), (what, top)
        finally:
            ctx.set_option("nn_lds_top", before)
        other = Cl.blob_tail(4) if cloud.name != Cl.blob_tail(4).name else Cl.blob_tail(0)
        ot, onl = self.fixed(other), fresh(other)["info"][1]
        if cloud.name not in self._ref:
            up = self.fixed(cloud)
            self._ref[cloud.name] = (self.register(up, ot, f["info"][1]), self.register(ot, up, onl))
        as_moving, as_fixed = self._ref[cloud.name]
        same_bits(self.register(tid, ot, f["info"][1]), as_moving, (what, "moving leaves from the built block"))
        same_bits(self.register(ot, tid, onl), as_fixed, (what, "screening records and staged top of the built block"))


def run(scenario, chains, vias=("sync",), between=None):
    """Every chain (A, B, ...) on one context per entry: A, then every later cloud TWICE in a row — the first time behind a
    wrong history, the second behind a right one."""
    for via in vias:
        ctx = capi.Context(0)
        try:
            h = History(ctx, scenario)
            for chain in chains:
                h.held(chain[0], via, records=False)
                for cloud in chain[1:]:
                    if between is not None:
                        between(ctx)
                    h.held(cloud, via)
                    h.held(cloud, via)
            print("scenario %s [%s]: %d builds held" % (scenario, via, h.pairs))
        finally:
            ctx.close()


BOTH = ("sync", "lookahead")


def test_1_dense_tree_behind_a_one_leaf_tree():
    """gauss40k at b_max 1e3 (one leaf), then at 1e-5 (40 000 leaves, depth 18).  `need` is 0 for every step, so every launch is
    cropped to 24 workgroups: the 42 team-regime nodes of level 6 share 23 of them (tb_level: wgT = min(cntT, G - 1), walked
    with a stride) and the one workgroup left does the wave AND the quad queue (`single`); 18 steps are launched and the tree
    is deeper: the continue-and-check loop of tree_build_end_on; the pre-sized block holds 257 leaves: tb_emit writes nothing
    and the host emits again."""
    run("1", [(Cl.gauss40k(1e3), Cl.gauss40k(1e-5))], BOTH)


def test_2_one_leaf_tree_behind_a_dense_tree():
    """The other way round: the pre-sized emission of a one-node tree into a block for 40 000 leaves, 39 999 stale internal
    nodes in the temporary array, a staged top of one entry — and the dense tree once more behind it."""
    run("2", [(Cl.gauss40k(1e-5), Cl.gauss40k(1e3), Cl.gauss40k(1e-5))], BOTH)


@pytest.mark.parametrize("u", Cl.DUPS_EDGE)
def test_3_leaf_count_at_the_edge_of_the_pre_sized_block(u):
    """dups(1000), then u = 1380, 1381, 1382 leaves: the block sized from 1 000 leaves holds 1 381 — one below, exactly at, one
    above (tb_emit: nl > leaf_cap writes nothing; tree_build_end_on: n_leaves <= pre_leaf_cap keeps the block)."""
    run("3", [(Cl.dups(1000), Cl.dups(u))])


def test_4_smaller_trees_behind_a_larger_one():
    """dups(1382), dups(1000), then 4 000 copies of one point: a generous block each time, the nodes and top records of a
    larger tree stale in the arrays."""
    run("4", [(Cl.dups(1382), Cl.dups(1000), Cl.dups(1))])
    ctx = capi.Context(0)
    try:
        h = History(ctx, "4")
        for c in (Cl.dups(1382), Cl.dups(1000), Cl.dups(1)):  # (... and without the second build in between)
            h.held(c, "sync")
    finally:
        ctx.close()


@pytest.mark.parametrize("via", BOTH)
@pytest.mark.parametrize("k_a", Cl.TAILS_A)
def test_5_depth_hint_wrong_both_ways(k_a, via):
    """blob_tail(k_a), depth 14, 16, 17, 18 -> 18, 18, 19, 20 steps launched for the build behind it, against trees of depth
    14 .. 29 with the same leaf count within a per cent: no extra round of eight steps, one, two; a pre-sized tree that fits
    and is dropped all the same because steps were added behind it (pre_steps != levels_done); `quiet_from` cropping steps
    that are not quiet."""
    a = Cl.blob_tail(k_a)
    run("5", [(a, Cl.blob_tail(k_b)) for k_b in Cl.TAILS_B], (via,))


def test_6_both_sides_of_similar():
    """Behind 4 000 points: 3 499 and 4 501 points forget every hint, 3 500 and 4 500 take them all."""
    run("6", [(Cl.blob_tail(0), Cl.blob_head(n)) for n in Cl.HEADS])


@pytest.mark.parametrize("via", BOTH)
def test_7_ten_rounds_of_the_continue_and_check_loop(via):
    """line2(-47, 47), depth 94: as the first build of the context (20 steps, then 76 more in rounds of eight, the summary redone
    every time), behind itself (a right hint that cannot help: 20 steps at most) and behind a one-leaf tree of the same 95
    points (18 steps first)."""
    deep = Cl.line2(*Cl.LINE_DEEP)
    run("7", [(deep, deep), (Cl.blob_head(95, 1e3), deep)], (via,))


def refused(h, cloud, via):
    with pytest.raises(capi.MadIcpError, match=r"madicp error -1: .*deeper than the supported 96 levels"):  # MADICP_ERR_INVALID
        h.build(cloud, via)
    print("scenario %s [%s] %s -> %s: refused" % (h.scenario, via, h.last, cloud.name))
    h.last = cloud.name + " (refused)"


def test_8_a_tree_too_deep_is_refused_and_leaves_nothing_behind():
    """A tree deeper than the builder supports is an error return — MADICP_ERR_INVALID, "deeper than the supported 96 levels" —
    from madicp_tree_build and from madicp_tree_build_end: no tree id is issued, and the builds behind it are their fresh
    builds: a cloud of the refused cloud's size (which would take its hints if it had left any), another size, the refused
    cloud again, another one.  The boundary: steps 0 .. kMaxLevels - 1 are launched and a node of level L is made by step
    L at the earliest, so depth 95 builds and depth 96 — nodes queued for step 96 — does not."""
    ctx = capi.Context(0)
    try:
        h = History(ctx, "8")
        deep = Cl.line2(*Cl.LINE_REFUSED)
        live = [h.held(Cl.blob_tail(8), "sync", keep=True)]
        refused(h, deep, "sync")
        live.append(h.held(Cl.blob_head(141), "sync", keep=True))
        live.append(h.held(Cl.blob_tail(8), "sync", keep=True))
        refused(h, deep, "lookahead")
        with pytest.raises(capi.MadIcpError, match="no look-ahead tree build in flight"):
            ctx.tree_build_end()
        live.append(h.held(Cl.blob_head(141), "lookahead", keep=True))
        live.append(h.held(Cl.dups(1000), "sync", keep=True))
        # either side of the limit, both entries
        at, past = Cl.line2(-48, 47), Cl.line2(-48, 48)
        assert at.pts.shape[0] == Cl.MAX_DEPTH + 1 and past.pts.shape[0] == Cl.MAX_DEPTH + 2
        for via in BOTH:
            live.append(h.held(at, via, keep=True))
            refused(h, past, via)
            live.append(h.held(at, via, keep=True))
        # the only trees of the context are the ones that were handed out
        assert len(set(live)) == len(live)
        live += list(h._fixed.values())  # (and the uploaded reference trees of the records checks)
        for i in range(max(live) + 16):
            if i in live:
                ctx.tree_info(i)
            else:
                with pytest.raises(capi.MadIcpError, match="unknown tree id"):
                    ctx.tree_info(i)
    finally:
        ctx.close()


def test_9_hints_survive_the_scratch_being_written_over():
    """Between A and B a 4 000-point cloud is deskewed and folded into a voxel map: both borrow idle parts of the builder's
    scratch.  The hints are the host's and survive; nothing the build reads may be what the borrowers left."""
    def between(ctx):
        cid = ctx.cloud_upload(Cl.blob_tail(0).pts + [30.0, 0.0, 0.0])
        mid = ctx.map_create(0.5, 64, 1 << 16)
        try:
            ctx.cloud_deskew(cid, [0.9, 0.05, 0.0, 0.0, 0.02, 0.03], 10.0)
            ctx.map_insert_cloud(mid, cid, np.eye(3), np.zeros(3))
        finally:
            ctx.map_release(mid)
            ctx.cloud_release(cid)

    run("9", [(Cl.gauss40k(1e3), Cl.gauss40k(1e-5)), (Cl.dups(1000), Cl.dups(1382)), (Cl.blob_tail(0), Cl.blob_tail(16))], between=between)


def test_10_a_cancelled_look_ahead_leaves_nothing_behind():
    """begin(A), cancel, B: neither A's hints (it never finished on the host) nor its pre-sized block; and begin(B), cancel,
    begin(B), end behind a finished A: the cancelled construction's pre-sized block goes back, the second one is A's successor."""
    a, b = Cl.blob_tail(0), Cl.blob_tail(16)
    for via in BOTH:
        ctx = capi.Context(0)
        try:
            h = History(ctx, "10")
            ctx.tree_build_begin(a.pts, a.b_max, a.b_min)
            ctx.tree_build_cancel()
            h.last = a.name + " (cancelled)"
            h.held(b, via)
            h.held(b, via)
            h.held(a, "lookahead", records=False)
            ctx.tree_build_begin(b.pts, b.b_max, b.b_min)
            ctx.tree_build_cancel()
            h.held(b, "lookahead")
            ctx.tree_build_begin(a.pts, a.b_max, a.b_min)
            ctx.tree_build_cancel()
            h.held(b, via)
        finally:
            ctx.close()
