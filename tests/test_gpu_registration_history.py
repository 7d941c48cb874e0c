"""A registration's outputs are a function of its arguments and the resident trees alone — whatever the moving set, the stream
slot or the context held before.

The registration side keeps more state between calls than any other part of the C ABI (madicp_capi.hip): DevMoving's device
blocks, matched flags and correspondence cache (reserve_moving, reserve_cache), a stream slot's pinned blocks (prepare_slot,
reserve_pinned_in; a submission sizes every idle slot of the ring), the context's partial rows and walk hints (ensure_partials;
zeroed by prepare_partials only when the launch geometry changes), the captured launch sequences (one graph replayed for every
L that yields the same plan), the Job staging ring, the publish ring, last_moving / last_batch.  tests/registration_history.py
drives all of it on ONE long-lived context — 66 steps: register, linearize, batch, pipelined batches, two streamed
registrations in flight, streamed registrations of resident moving trees, each kind walking the size list 1, c(1), c(1)+1,
c(c(1)+1), c(c(1)+1)+1, 65, L_full, 64, 1, c(1)+1, L_full-1 on ids of its own — and every step is held, BYTE FOR BYTE (X, H, b,
matched flags, X_iters, visits, accepted pairs, correspondences), to the same call made alone on a fresh context whose moving
sets were created at the step's sizes.  That the list crosses the capacities and the plans reuse graphs, shrink grids and grow
the partial block is held on the CPU (tests/test_registration_history_inputs.py).

Anchors that do not pass through the code under test: the fresh registration of a whole scan is the oracle's to the
POSE_TOL_* of tests/test_gpu_parity.py, the fresh linearisation of a whole scan has the oracle's correspondences and gate
decisions bit for bit, and — correspondences are per leaf — every linearisation of a prefix on the long-lived context has
corr[k][:L] and matched[:L] of the whole scan's.

The sequence runs three times, each on a long-lived context of its own: default options, use_graph = 0, eager_when_busy = 0
(both claimed bit-neutral; the fresh side always runs under defaults and is computed once per distinct call).
Measured on MI355X (the tests print their times under -s): the default run 2.3 s, of which 1.9 s are the fresh contexts (77 at the most: 66
steps, the batch in the middle of a stream step, the whole-scan linearisations of the prefix anchor); use_graph = 0: 0.08 s;
eager_when_busy = 0: 0.12 s; the reuse check under 1 s.  No step differs from its fresh self.

What bites (scratch builds of madicp_capi.hip with value-only edits, never committed): prepare_partials without its memset on a
geometry change — 52 of the 67 compared results differ, from step 4 on; stage_registration without the single-round `matched`
memset — 9 of the 11 linearisations differ in `matched`, 8 of them also from the whole scan's prefix; reserve_moving keeping
cache_cap across a re-allocation (blocks of the right size) — nothing, and nothing can: icp_round reads the cache only when
round > 0 and round 0 writes every pair's entry.  An edit that leaves a freed or undersized pointer in use (reserve_moving
without the fence event, or keeping cap_L; reserve_cache trusting a stale cache_cap with the old blocks) was not run: the first
would let a pooled block be handed out while a registration in flight still reads it, the others write past a block."""
import contextlib
import time

import numpy as np
import pytest

import oracle_lib as O
import registration_history as RH
from fixtures import B_MAX, B_MIN, B_RATIO, PARAMS, RHO_KER
from mad_icp_amd import capi
from test_gpu_parity import POSE_TOL_M, POSE_TOL_RAD, pose_err

pytestmark = pytest.mark.gpu

_FRESH = {}     # Spec -> what the call gave alone on a fresh context
_ORACLE = {}


def oracle():
    """the oracle's trees of the scene: keyframes at their poses, the query scans in the sensor frame"""
    if not _ORACLE:
        pb = RH.problem()
        fixed = []
        for s, T in zip(pb.kf_scans, pb.kf_poses):
            t = O.Tree(s, B_MAX, B_MIN, 1)
            t.transform(T[:3, :3], T[:3, 3])
            fixed.append(t)
        _ORACLE.update(fixed=fixed, moving=[O.Tree(s, B_MAX, B_MIN, 1) for s in pb.q_scans])
        for q, m in enumerate(_ORACLE["moving"]):   # (the moving sets ARE the oracle's leaves: the host builder is its twin)
            assert m.leaves()[0].tobytes() == pb.leaves[q].tobytes()
    return _ORACLE


def hold_to_oracle(sp, r):
    """a fresh result whose moving set is a whole query scan, against the oracle"""
    (q, L), = sp.batches[0]
    pb, orc = RH.problem(), oracle()
    fixed = [orc["fixed"][k] for k in RH.tree_order(q)[:sp.Ks[0]]]
    if sp.kind == "register":
        o = O.icp_register(orc["moving"][q], fixed, pb.q_guess[q], RH.N_ITERS, B_MAX, RHO_KER, B_RATIO)
        dt, da = pose_err(o["T"], capi.pose44(r["X"]))
        assert dt <= POSE_TOL_M and da <= POSE_TOL_RAD, (sp, dt, da)
        for it in range(RH.N_ITERS):
            dt, da = pose_err(O.pose44(o["X_iters"][it]), capi.pose44(r["X_iters"][it]))
            assert dt <= POSE_TOL_M and da <= POSE_TOL_RAD, (sp, it, dt, da)
    else:
        matched, visits = np.zeros(L, np.uint8), 0
        for k, f in enumerate(fixed):
            _, _, corr, rej, mat, depth = O.icp_linearize(orc["moving"][q], f, pb.q_guess[q], B_MAX, RHO_KER, B_RATIO)
            assert np.array_equal(r["corr"][k] & 0x7FFFFFFF, corr), (sp, k)
            assert np.array_equal((r["corr"][k] >> 31).astype(np.uint8), rej), (sp, k)
            matched |= mat
            visits += depth
        assert np.array_equal(r["matched"], matched) and int(r["visits"][0]) == visits, sp


def fresh(sp):
    """the call alone: a new context with the same trees uploaded, moving sets created at the call's sizes; closed before the
    next one opens"""
    if sp not in _FRESH:
        with contextlib.closing(capi.Context(0)) as ctx:
            runner = RH.Runner(ctx, long_lived=False)
            (_, r), = runner.run(sp)
            runner.close()
        if sp.kind in ("register", "linearize") and sp.batches[0][0][1] == RH.l_full(sp.batches[0][0][0]):
            hold_to_oracle(sp, r)
        _FRESH[sp] = r
    return _FRESH[sp]


def same_bytes(got, want, where):
    assert got.keys() == want.keys(), where
    for name in got:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, where + (name,)
        assert got[name].tobytes() == want[name].tobytes(), where + (name,)


def run_sequence(options):
    t0 = time.perf_counter()
    t_fresh = 0.0
    with contextlib.closing(capi.Context(0)) as ctx:
        saved = {k: ctx.get_option(k) for k in options}
        for k, v in options.items():
            ctx.set_option(k, v)
        shared = RH.Runner(ctx, long_lived=True)
        for step, kind, n in RH.STEPS:
            for sp, got in shared.run(RH.spec_of(kind, n)):
                t1 = time.perf_counter()
                want = fresh(sp)
                t_fresh += time.perf_counter() - t1
                same_bytes(got, want, (step, kind, n, sp.kind))
                if sp.kind == "linearize":   # per leaf: a prefix's correspondences are the whole scan's
                    (q, L), = sp.batches[0]
                    t1 = time.perf_counter()
                    whole = fresh(sp._replace(batches=(((q, RH.l_full(q)),),)))
                    t_fresh += time.perf_counter() - t1
                    assert got["corr"].shape == (sp.Ks[0], L) and got["corr"].tobytes() == whole["corr"][:, :L].tobytes(), (step, L)
                    assert got["matched"].tobytes() == whole["matched"][:L].tobytes(), (step, L)
        for k, v in saved.items():
            ctx.set_option(k, v)
        shared.close()     # every moving id and every tree released: both must succeed on a context with this history
        ctx.synchronize()
    total = time.perf_counter() - t0
    print("registration history %r: %.2f s, of which %.2f s on fresh contexts" % (options, total, t_fresh))


def test_every_step_is_the_call_alone_on_a_fresh_context(natives):
    run_sequence({})


def test_the_same_without_graphs(natives):
    run_sequence({"use_graph": 0})


def test_the_same_with_graphs_behind_a_busy_stream(natives):
    run_sequence({"eager_when_busy": 0})


def test_correspondence_reuse_is_at_work_at_these_shapes(natives):
    """A whole scan against nine trees, four rounds: rounds 1 to 3 reuse correspondences — the cache that reserve_moving /
    reserve_cache re-allocate is in use — and give the same bits as with option cache_correspondences = 0.  `visits` is the
    REFERENCE's count (a reused pair counts the depth it was found at: tests/test_gpu_parity.py holds it to the oracle), so it is
    equal either way; what reuse saves shows in Job::walked, the nodes really walked, which the measurement build reports."""
    sp = RH.Spec("register", (((0, RH.l_full(0)),),), (9,), (), None)
    with contextlib.closing(capi.Context(0)) as ctx:
        runner = RH.Runner(ctx, long_lived=False)
        (_, cached), = runner.run(sp)
        ctx.set_option("cache_correspondences", 0)
        (_, rewalked), = runner.run(sp)
        ctx.set_option("cache_correspondences", 1)
        runner.close()
    print("visits with reuse %d, without %d" % (cached["visits"][0], rewalked["visits"][0]))
    same_bytes(cached, rewalked, ("reuse",))
    mc = capi.measure_variant()
    if not hasattr(mc.hip_lib(), "madicp_icp_time_registration"):
        pytest.skip("this build of the library has no measurement aids (a variant run without -DMADICP_MEASURE)")
    pb = RH.problem()
    with contextlib.closing(mc.Context(0)) as ctx:
        tids = [ctx.upload(pb.kf_trees[k]) for k in RH.tree_order(0)]
        mid = ctx.moving_upload(pb.leaves[0])
        walked = {}
        for on in (1, 0):
            ctx.set_option("cache_correspondences", on)
            _, _, visits, w = ctx.icp_time_registration([mid], tids, capi.pose12(pb.q_guess[0])[None], PARAMS, RH.N_ITERS, reps=1)
            walked[on] = (int(visits[0]), int(w[0]))
        ctx.set_option("cache_correspondences", 1)
        ctx.moving_release(mid)
        for t in tids:
            ctx.tree_release(t)
    print("per round (visits, walked): with reuse %r, without %r" % (walked[1], walked[0]))
    assert walked[1][0] == walked[0][0] == int(cached["visits"][0]) // RH.N_ITERS
    assert walked[0][1] == walked[0][0]                  # without reuse every visited node is walked
    assert walked[1][1] < walked[0][1], walked           # with it, rounds 1 to 3 walk less
