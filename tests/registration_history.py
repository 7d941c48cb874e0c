"""Inputs, call kinds and the sequence of tests/test_gpu_registration_history.py; the preconditions the sequence rests on are
held on the CPU by tests/test_registration_history_inputs.py.

The registration side of the C ABI keeps state between calls (mad_icp_amd/csrc/hip/madicp_capi.hip): a moving set's device
blocks, flags and correspondence cache grow by `reserve_moving` / `reserve_cache`, a stream slot's pinned blocks by
`prepare_slot`, the context's partial rows by `ensure_partials` (zeroed by `prepare_partials` only when the launch geometry
changes) and captured launch sequences are replayed for every L that yields the same plan.  The sequence below drives all of
it on ONE context: six kinds of call, each on long-lived moving ids (or the stream ring) of its own, each walking the same
list of sizes — so that every id meets "exactly full", "one past", "a jump up", "a large buffer used small" in that order.

A moving set is any (L, 3) array: PREFIXES of a query scan's leaf means reach exact sizes.  With c(L) the capacity rule of
reserve_moving (read from the source, see capacity_rule) the list is

    1, c(1), c(1)+1, c(c(1)+1), c(c(1)+1)+1, 65, L_full, 64, 1, c(1)+1, L_full-1

Every kind's n-th occurrence takes entry n as its first size (a batch's scan s takes entry n + s, the second of two batches or
submissions in flight the entries after it), K cycles through 1, 9, 2, 8 and B through 1, 3, 8 with the occurrence: 11, 4 and 3
are pairwise coprime, and the six kinds take turns, so 66 steps meet every kind with every entry of the list once."""
import collections
import functools
import os
import re
import subprocess

import numpy as np

from fixtures import B_MAX, B_MIN, PARAMS
from mad_icp_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI_HIP = os.path.join(ROOT, "mad_icp_amd", "csrc", "hip", "madicp_capi.hip")

SEED = 1
N_KEYFRAMES, N_QUERIES = 9, 3
N_ITERS = 4
KINDS = ("register", "linearize", "batch", "pipelined", "stream", "stream_tree")
K_CYCLE = (1, 9, 2, 8)
B_CYCLE = (1, 3, 8)
N_SIZES = 11
N_STEPS = len(KINDS) * N_SIZES
MID_BATCH_AT = 0        # the occurrence of "stream" that has a batch of 8 between its submissions and its collects
FULL, FULL_LESS_ONE = "full", "full-1"   # list entries that follow the scan: its leaf count, and one less
# strides of the two resident moving trees of "stream_tree" by occurrence: few leaves while the ring is small
STRIDES = ((40, 24), (24, 12), (12, 10), (10, 7), (7, 3), (3, 2), (2, 1), (5, 1), (40, 2), (1, 24), (7, 12))
N_STREAM_SLOTS = 4      # madicp_ctx::kStreamSlots


# ---- constants read from the source ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capacity_rule():
    """The `cap` expression of reserve_moving, as text (the sizes follow it; the CPU test pins it)."""
    src = open(CAPI_HIP).read()
    body = src[src.index("int reserve_moving("):]
    body = body[:body.index("\nint reserve_cache(")]
    m = re.findall(r"const int cap = ([L0-9 +*/()]+);", body)
    assert len(m) == 1, "reserve_moving no longer has one `const int cap = <expression in L>;`"
    return m[0].strip()


def c(L):
    """capacity of a moving set re-allocated for L leaves (C integer arithmetic on non-negative values)"""
    return int(eval(capacity_rule().replace("/", "//"), {"__builtins__": {}}, {"L": int(L)}))


def sizes():
    """the list, with the two entries that follow the scan left symbolic"""
    a = c(1)
    b = c(a + 1)
    return (1, a, a + 1, b, b + 1, 65, FULL, 64, 1, a + 1, FULL_LESS_ONE)


# ---- the scene ------------------------------------------------------------------------------------------------------------------
Problem = collections.namedtuple("Problem", "kf_scans kf_poses kf_trees q_scans q_gt q_guess q_s leaves")


@functools.lru_cache(maxsize=None)
def problem():
    """The fuzz test's scene at its resolution: nine keyframes 1.5 m apart, host-built and moved to their poses, three query
    scans between them with guesses a few centimetres from the truth."""
    scene = synth.Scene(SEED)
    kf_poses = [synth.path_pose(1.5 * k) for k in range(N_KEYFRAMES)]
    kf_scans = [synth.render_scan(scene, T, 40 + k, n_beams=16, n_azimuth=300) for k, T in enumerate(kf_poses)]
    kf_trees = []
    for s, T in zip(kf_scans, kf_poses):
        ht = capi.HostTree(s, B_MAX, B_MIN, 1)
        ht.transform(T[:3, :3], T[:3, 3])
        kf_trees.append(ht)
    q_s = (5.3, 6.1, 7.4)
    q_gt = [synth.path_pose(s) for s in q_s]
    q_scans = [synth.render_scan(scene, T, 90 + q, n_beams=16, n_azimuth=300) for q, T in enumerate(q_gt)]
    q_guess = [T @ synth.perturbation(900 + q, trans=0.04, rot_deg=0.3) for q, T in enumerate(q_gt)]
    leaves = [capi.HostTree(s, B_MAX, B_MIN, 1).leaf_means() for s in q_scans]
    return Problem(kf_scans, kf_poses, kf_trees, q_scans, q_gt, q_guess, q_s, leaves)


def l_full(q):
    return problem().leaves[q].shape[0]


def size_of(entry, q):
    return l_full(q) if entry == FULL else l_full(q) - 1 if entry == FULL_LESS_ONE else entry


def tree_order(q):
    """the keyframes, nearest to query q first: a registration against K trees takes the first K"""
    return tuple(sorted(range(N_KEYFRAMES), key=lambda k: abs(1.5 * k - problem().q_s[q])))


@functools.lru_cache(maxsize=None)
def moving_tree(q, stride):
    """host-built tree of every stride-th point of query scan q (sensor frame): a resident moving tree of "stream_tree" """
    return capi.HostTree(np.ascontiguousarray(problem().q_scans[q][::stride]), B_MAX, B_MIN, 1)


# ---- the sequence ---------------------------------------------------------------------------------------------------------------
# One call of the sequence.  batches: for every batch (or submission) in flight, its scans as (query, L); Ks: trees per batch or
# submission; strides: the resident moving trees of "stream_tree" (submitted BEFORE its leaf-means submission); mid: the batch
# run between a stream step's submissions and its collects.
Spec = collections.namedtuple("Spec", "kind batches Ks strides mid")


def _scan(n, s=0):
    q = (n + s) % N_QUERIES
    return q, size_of(sizes()[(n + s) % N_SIZES], q)


def spec_of(kind, n):
    """the n-th occurrence of a kind"""
    K, B = K_CYCLE[(n + KINDS.index(kind)) % len(K_CYCLE)], B_CYCLE[(n + KINDS.index(kind) + 1) % len(B_CYCLE)]
    if kind in ("register", "linearize"):
        return Spec(kind, ((_scan(n),),), (K,), (), None)
    if kind == "batch":
        return Spec(kind, (tuple(_scan(n, s) for s in range(B)),), (K,), (), None)
    if kind == "pipelined":   # two batches on two sets of ids: batch j of the kind walks the list from entry j
        return Spec(kind, tuple(tuple(_scan(2 * n + j, s) for s in range(B)) for j in (0, 1)), (K, K), (), None)
    if kind == "stream":      # two submissions in flight with different L and K
        K2 = K_CYCLE[(n + KINDS.index(kind) + 1) % len(K_CYCLE)]
        mid = Spec("batch", (tuple(_scan(3, s) for s in range(8)),), (2,), (), None) if n == MID_BATCH_AT else None
        return Spec(kind, ((_scan(n),), (_scan(n + 1),)), (K, K2), (), mid)
    q = n % N_QUERIES         # (its leaf-means submission takes the entry after the two that "stream" has just had)
    return Spec(kind, ((_scan(n + 2),),), (K,), tuple((q, s) for s in STRIDES[n]), None)


STEPS = tuple((i, KINDS[i % len(KINDS)], i // len(KINDS)) for i in range(N_STEPS))   # (step, kind, occurrence)


def specs():
    return [spec_of(kind, n) for _, kind, n in STEPS]


# ---- the call kinds -------------------------------------------------------------------------------------------------------------
def _u64(v):
    return np.array([v], np.uint64)


def initial_leaves(name):
    """what a long-lived id holds when it is created (census() starts from the same)"""
    pb = problem()
    return pb.leaves[0] if name[0] in ("batch", "pipe0", "pipe1") and name[1] >= 5 else pb.leaves[0][:1]


class Runner:
    """The six kinds on one context.  long_lived: moving sets are ids created once (a single leaf; the last sets of a batch of
    eight at full size: "created large and never grown") and rewritten by madicp_moving_update / _update_async — the context
    under test.  Otherwise every set is created by madicp_moving_upload at the size the call needs and "pipelined" is the
    synchronous update -> enqueue -> fetch of the same batches: the same call ALONE, on a context that holds nothing else."""

    def __init__(self, ctx, long_lived):
        self.ctx, self.long_lived = ctx, long_lived
        pb = problem()
        self.tids = [ctx.upload(ht) for ht in pb.kf_trees]
        self.ids = {}

    def put(self, name, q, L, asynchronous=False):
        m = problem().leaves[q][:L]
        if not self.long_lived:
            if name in self.ids:
                self.ctx.moving_release(self.ids.pop(name))
            self.ids[name] = self.ctx.moving_upload(m)
            return self.ids[name]
        if name not in self.ids:
            self.ids[name] = self.ctx.moving_upload(initial_leaves(name))
        (self.ctx.moving_update_async if asynchronous else self.ctx.moving_update)(self.ids[name], m)
        return self.ids[name]

    def trees(self, q, K):
        return [self.tids[k] for k in tree_order(q)[:K]]

    def close(self):
        """every moving id and every tree is released; the caller closes the context"""
        for mid in self.ids.values():
            self.ctx.moving_release(mid)
        for tid in self.tids:
            self.ctx.tree_release(tid)
        self.ids, self.tids = {}, []

    # every kind: Spec -> [(Spec, dict of arrays)] — a stream step with a batch in its middle answers for both
    def run(self, sp):
        return getattr(self, "_" + sp.kind)(sp)

    def _register(self, sp):
        (q, L), = sp.batches[0]
        mid = self.put(("reg", 0), q, L)
        r = self.ctx.icp_register(mid, self.trees(q, sp.Ks[0]), problem().q_guess[q], PARAMS, N_ITERS, L)
        return [(sp, dict(X=r["X"], H=r["H"], b=r["b"], matched=r["matched"], X_iters=r["X_iters"], visits=_u64(r["visits"])))]

    def _linearize(self, sp):
        (q, L), = sp.batches[0]
        mid = self.put(("lin", 0), q, L)
        r = self.ctx.icp_linearize(mid, self.trees(q, sp.Ks[0]), problem().q_guess[q], PARAMS, L)
        return [(sp, dict(corr=r["corr"], H=r["H"], b=r["b"], matched=r["matched"], visits=_u64(r["visits"])))]

    def _enqueue(self, prefix, scans, K, asynchronous=False):
        mids = [self.put((prefix, s), q, L, asynchronous) for s, (q, L) in enumerate(scans)]
        X0 = np.stack([capi.pose12(problem().q_guess[q]) for q, _ in scans])
        self.ctx.icp_register_batch_enqueue(mids, self.trees(scans[0][0], K), X0, PARAMS, N_ITERS)

    def _fetched(self, r, scans, tag=""):
        out = {tag + k: r[k] for k in ("X", "H", "b", "n_matched", "visits")}
        if scans is not None:
            for s, (_, L) in enumerate(scans):
                out["%smatched%d" % (tag, s)] = self.ctx.icp_fetch_matched(s, L)
        return out

    def _batch(self, sp, prefix="batch"):
        scans = sp.batches[0]
        self._enqueue(prefix, scans, sp.Ks[0])
        return [(sp, self._fetched(self.ctx.icp_fetch(len(scans)), scans))]

    def _pipelined(self, sp):
        a, b = sp.batches
        out = {}
        if not self.long_lived:
            for tag, scans in (("a_", a), ("b_", b)):
                self._enqueue("pipe" + tag, scans, sp.Ks[0])
                out.update(self._fetched(self.ctx.icp_fetch(len(scans)), scans if tag == "b_" else None, tag))
            return [(sp, out)]
        tickets = []
        for j, scans in enumerate((a, b)):   # batch a's results are collected after batch b has been uploaded and enqueued
            self._enqueue("pipe%d" % j, scans, sp.Ks[0], asynchronous=True)
            tickets.append(self.ctx.icp_publish_enqueue(len(scans)))
        out.update(self._fetched(self.ctx.icp_publish_collect(tickets[0], len(a)), None, "a_"))
        out.update(self._fetched(self.ctx.icp_publish_collect(tickets[1], len(b)), b, "b_"))   # (flags: the batch enqueued last)
        return [(sp, out)]

    def _collect(self, tickets, Ls):
        out = {}
        for i, (tk, L) in enumerate(zip(tickets, Ls)):
            r = self.ctx.stream_collect(tk, L)
            out.update({"%s%d" % (k, i): r[k] for k in ("X", "H", "b", "matched")})
            out["n_matched%d" % i], out["visits%d" % i] = np.array([r["n_matched"]], np.int32), _u64(r["visits"])
        return out

    def _submit(self, q, L, K):
        pb = problem()
        return self.ctx.stream_submit(pb.leaves[q][:L], self.trees(q, K), pb.q_guess[q], PARAMS, N_ITERS)

    def _stream(self, sp):
        scans = [b[0] for b in sp.batches]
        tickets = [self._submit(q, L, K) for (q, L), K in zip(scans, sp.Ks)]
        # (the partial rows grow — the block is freed, every captured graph dropped — with two tickets pending)
        mid = self._batch(sp.mid, prefix="mid") if sp.mid is not None and self.long_lived else []
        return [(sp._replace(mid=None), self._collect(tickets, [L for _, L in scans]))] + mid

    def _stream_tree(self, sp):
        (q, L), = sp.batches[0]
        pb = problem()
        hts = [moving_tree(tq, s) for tq, s in sp.strides]
        mtids = [self.ctx.upload(ht) for ht in hts]
        try:
            tickets = [self.ctx.stream_submit_tree(t, self.trees(tq, sp.Ks[0]), pb.q_guess[tq], PARAMS, N_ITERS)
                       for t, (tq, _) in zip(mtids, sp.strides)]
            tickets.append(self._submit(q, L, sp.Ks[0]))   # the ring's pinned input blocks are first needed now
            return [(sp, self._collect(tickets, [ht.num_leaves for ht in hts] + [L]))]
        finally:
            for t in mtids:
                self.ctx.tree_release(t)


# ---- what the sequence does to the retained state, simulated on the host --------------------------------------------------------
Launch = collections.namedtuple("Launch", "step kind max_L K batch iters trace slot")


def census():
    """The capacity of every long-lived moving id and of every stream slot along the sequence, by reserve_moving's rule and
    stream_submit_impl's "a submission sizes its slot and every idle slot".  Returns (events, launches):
    events    (step, kind, path, what): path "update" / "update_async" / "slot" / "slot_idle"; what "exact" (L equals the capacity: no
              re-allocation), "fits", "past" (L is the capacity + 1: re-allocation) or "jump" (re-allocation by more)
    launches  every registration in the order the long-lived context enqueues them (Launch)"""
    caps, slot_cap, pending, ticket = {}, [0] * N_STREAM_SLOTS, [False] * N_STREAM_SLOTS, [0]
    events, launches = [], []

    def what(L, cap):
        return "exact" if L == cap else "fits" if L < cap else "past" if L == cap + 1 else "jump"

    def update(step, kind, name, L, path):
        if name not in caps:
            caps[name] = c(initial_leaves(name).shape[0])
        events.append((step, kind, path, what(L, caps[name])))
        if L > caps[name]:
            caps[name] = c(L)

    def submit(step, kind, L, K):
        own = ticket[0] % N_STREAM_SLOTS
        assert not pending[own]
        for j in range(N_STREAM_SLOTS):
            if j == own or not pending[j]:
                if slot_cap[j]:   # (the first sizing of a slot re-allocates nothing)
                    w = what(L, slot_cap[j])
                    if j == own or w in ("past", "jump"):
                        events.append((step, kind, "slot" if j == own else "slot_idle", w))
                if L > slot_cap[j]:
                    slot_cap[j] = c(L)
        launches.append(Launch(step, kind, L, K, 1, N_ITERS, 0, own))
        pending[own] = True
        ticket[0] += 1
        return own

    def batch(step, kind, prefix, scans, K, path):
        for s, (_, L) in enumerate(scans):
            update(step, kind, (prefix, s), L, path)
        launches.append(Launch(step, kind, max(L for _, L in scans), K, len(scans), N_ITERS, 0, -1))

    for step, kind, n in STEPS:
        sp = spec_of(kind, n)
        if kind in ("register", "linearize"):
            (_, L), = sp.batches[0]
            update(step, kind, (kind[:3], 0), L, "update")
            launches.append(Launch(step, kind, L, sp.Ks[0], 1, N_ITERS if kind == "register" else 1, int(kind == "linearize"), -1))
        elif kind == "batch":
            batch(step, kind, "batch", sp.batches[0], sp.Ks[0], "update")
        elif kind == "pipelined":
            for j, scans in enumerate(sp.batches):
                batch(step, kind, "pipe%d" % j, scans, sp.Ks[0], "update_async")
        elif kind == "stream":
            own = [submit(step, kind, b[0][1], K) for b, K in zip(sp.batches, sp.Ks)]
            if sp.mid is not None:
                batch(step, "batch(mid)", "mid", sp.mid.batches[0], sp.mid.Ks[0], "update")
            for j in own:
                pending[j] = False
        else:
            own = [submit(step, kind, moving_tree(tq, s).num_leaves, sp.Ks[0]) for tq, s in sp.strides]
            own.append(submit(step, kind, sp.batches[0][0][1], sp.Ks[0]))
            for j in own:
                pending[j] = False
    return events, launches


def plans(launches, exe):
    """make_plan for every launch through tests/cpp/registration_history_plan.cpp built as `exe`: (floor of ensure_partials,
    [(grid, partial doubles, tie)])"""
    text = "".join("%d %d %d %d %d\n" % (l.max_L, l.K, l.batch, l.iters, l.trace) for l in launches)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    rows = [r.split() for r in out[1:] if r]
    assert len(rows) == len(launches)
    return int(out[0]), [(int(g), int(d), t) for g, d, t in rows]
