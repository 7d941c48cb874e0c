"""The device's Gauss-Newton update step — solve_pose of mad_icp_amd/csrc/hip/kernels.hip.h: the lane-parallel Gauss-Jordan
gn_solve_lanes (under -DMADICP_EXACT_SOLVE the restated ldlt6_solve), exp_so3 with its three branches, the pose composition
and the moved[] bounds that correspondence and gate reuse rely on — held to an exact solve of its own inputs.

`madicp_icp_register` with n_iters = r returns the joined H, b of round r - 1 (the very bits solve_pose read in icp_final),
the pose before that round (X_iters[r - 1]) and the pose after it (X): the update X0, H, b -> X1 has bit-known inputs, and
tests/gn_step_ref.py computes it with mpmath at 256 bits (held to the oracle's double LDLT and expMapSO3 on a CPU by
tests/test_gn_step_ref.py).  The scenes (gn_step_ref.case) are tiny clouds built to reach what the street registrations never
do: steps on all three branches of exp_so3, translation- and rotation-led pivot orders (nine distinct orders at the first
round, more in the rounds after), an exact tie on the diagonal, cond(H) of 3e4, a scaled condition number of 9e5, Huber
weights on every pair, H with three rows that are exactly zero, and H = 0.  Every scene is asserted to be in its regime from the
device's own H, b (gn_step_ref.check_conditions).

Error measure: err(dx) = |D (dx - dx_exact)| / |D dx_exact|, D = sqrt(diag H).  dx_dev is recovered from the poses in high
precision (gn_step_ref.recover).  Bound: err(dx_dev) <= c kappa_s 2^-53 with kappa_s = cond(D^-1 H D^-1) and c = 8 rho_ref,
rho_ref being the oracle's own largest err / (kappa_s 2^-53) over these scenes — measured, not picked: rho_ref = 0.50, c = 4.0
(tests/test_gn_step_ref.py prints both).  Every entry of X1 must lie within that bound, propagated, plus 4 2^-53 (1 + |t0|)
for the double composition, of the reference's X1.  In the rounds after the first the steps shrink to 1e-7 and below, where
the composition's rounding is a visible fraction of the step: there the recovered dx is allowed that rounding on top
(gn_step_ref.bounds; the product's own host update in double needs it, see tests/test_gn_step_ref.py).  Plainly: from about the
fourth round on that allowance is thousands of times c kappa_s 2^-53, the dx assertion no longer constrains the solver, and the
OPERATIVE check of a later round is the one on the entries of X1 (4 2^-53 (1 + |t0|) plus the propagated bound) — a departure
from "the step within the bound" read as a bound on the recovered dx, which no update computed in doubles can meet there.

The exact tie H_00 == H_11 ("diagonal tie") shows that tied diagonal entries get two different ranks and the solve stays right:
a ballot that gave both rows one rank would drop an unknown.  WHICH of the two the device takes first cannot be seen from X1
(either order is a valid pivoting of the same system); "ties to the lower index" is the reference's order, computed by
gn_step_ref.pivot_order, not something asserted of the device.

Measured on an MI355X, err(dx_dev) / (kappa_s 2^-53) at the first round (c = 4.01), default build / -DMADICP_EXACT_SOLVE build:
large step (libm, order 1 0 2 5 4 3) 0.11 / 0.05; mid step (sin_small, 5 3 4 1 0 2) 0.19 / 0.29; first-order (3 5 4 0 2 1)
0.03 / 0.24; big room (5 4 3 0 1 2) 0.22 / 0.55; lever arm (5 4 3 1 2 0) 0.03 / 0.09; Huber-dominant (3 5 4 2 0 1) 0.10 / 0.17;
Huber one face (3 5 4 2 1 0) 0.13 / 0.10; one plane (3 4 2 0 1 5) 0.01 / 0.05; diagonal tie (5 4 3 0 1 2) 0.15 / 0.29; no
matches 0 / 0.  Largest: 0.22 for the default build, 0.55 for the exact-solve build — the oracle's own is 0.50.  The entries of
X1 stay within 0.25 of their tolerance in every round of either build (0.02 / 0.05 at the first).
"""
import types

import numpy as np
import pytest

import gn_step_ref as G
import oracle_lib as O
from mad_icp_amd import capi

pytestmark = pytest.mark.gpu

LATER = ("large step", "lever arm", "Huber-dominant")
SINGLE_ROUND = ("one plane", "diagonal tie")   # (after one round their H is singular to rounding, not exactly: nothing to hold a step to)
KEYS = ("X", "X_iters", "H", "b", "matched")


def c_bound():
    return 8.0 * G.rho_ref()


@pytest.fixture(scope="module")
def scenes(ctx):
    made = {}

    def get(name):
        if name not in made:
            cs = G.case(name)
            of, om = G.oracle_trees(name)
            hf = capi.HostTree(cs["fixed"], G.TREE_B_MAX, G.TREE_B_MIN, 2)
            hm = capi.HostTree(cs["moving"], G.TREE_B_MAX, G.TREE_B_MIN, 2)
            assert np.array_equal(hf.nodes["mean"], of.export()["mean"])   # identical trees, or the bit-for-bit bars mean nothing
            assert np.array_equal(hm.leaf_means(), om.leaves()[0])
            leaf = hf.nodes["right"] == 0
            normals = np.empty((hf.num_leaves, 3))
            normals[hf.nodes["leaf_id"][leaf]] = hf.nodes["dir"][leaf]
            assert np.array_equal(normals, of.leaves()[1])
            made[name] = types.SimpleNamespace(name=name, T0=cs["T0"], params=cs["params"], of=of, om=om, L=hm.num_leaves,
                                               tid=ctx.tree_upload(hf.nodes, hf.num_leaves),
                                               mid=ctx.moving_upload(hm.leaf_means()), moving_leaves=hm.leaf_means())
        return made[name]

    yield get
    for s in made.values():
        ctx.tree_release(s.tid)
        ctx.moving_release(s.mid)


def register(ctx, s, n_iters, T=None):
    return ctx.icp_register(s.mid, [s.tid], s.T0 if T is None else T, s.params, n_iters, s.L)


def check_inputs_at(ctx, s, T):
    """correspondences, gate bits and the visit count at pose T against the oracle's, bit for bit"""
    g = ctx.icp_linearize(s.mid, [s.tid], T, s.params, s.L)
    H, b, corr, rej, mat, depth = O.icp_linearize(s.om, s.of, T, *s.params)
    assert np.array_equal(g["corr"][0] & 0x7FFFFFFF, corr)
    assert np.array_equal((g["corr"][0] >> 31).astype(np.uint8), rej)
    assert np.array_equal(g["matched"], mat) and g["visits"] == depth
    return G.sym(H), b, mat


def check_step(H, b, X0, X1, later=False):
    """The update X0, H, b -> X1 against the exact solve of H, b.  -> (reference, err(dx_dev) / (kappa_s u), largest
    |X1 - X1_ref| / tolerance)"""
    assert np.isfinite(H).all() and np.isfinite(b).all() and np.isfinite(X1).all()
    ref = G.step(H, b, X0)
    beta, slack, x1_tol = G.bounds(ref, X0, c_bound())
    e = G.err(ref, G.recover(X0, X1, ref["branch"] == "first-order"))
    x1 = float((np.abs(X1 - ref["X164"]) / x1_tol).max())
    ratio = e / (ref["kappa_s"] * G.U)
    print("  %s |w| %.3g order %s kappa_s %.3g: err(dx_dev) = %.3g = %.3f kappa_s u (c = %.2f%s); X1 within %.3f of its tolerance"
          % (ref["branch"], ref["theta"], ref["order"], ref["kappa_s"], e, ratio, c_bound(),
             ", + %.2g for the composition" % (slack / (ref["kappa_s"] * G.U)) if later else "", x1))
    assert e <= beta + (slack if later else 0.0), (e, beta, slack)
    assert x1 <= 1.0, np.abs(X1 - ref["X164"]) / x1_tol
    # where H has a row of zeros the unknown stays exactly zero (Eigen's LDLT; both device solvers): seen through the composition
    dead = [i for i in range(6) if i not in ref["live"]]
    if dead and ref["branch"] == "first-order" and np.array_equal(X0[:9], np.eye(3).reshape(-1)):
        for i in dead:
            if i < 3:
                assert X1[9 + i] == X0[9 + i], i                       # t1_i = t0_i + dx_i
            else:
                j, k = [(5, 7), (2, 6), (1, 3)][i - 3]                 # I + skew(w): the two entries that hold +-w_i
                assert X1[j] == 0.0 and X1[k] == 0.0, i
    return ref, ratio, x1


@pytest.mark.parametrize("name", G.CASES)
def test_first_round_inputs_and_step(ctx, scenes, name, capsys):
    s = scenes(name)
    r = register(ctx, s, 1)
    assert np.array_equal(r["X_iters"][0], O.pose12(s.T0))
    Ho, bo, mat = check_inputs_at(ctx, s, s.T0)
    assert np.array_equal(r["matched"], mat)
    assert np.array_equal(r["H"], r["H"].T)
    assert np.allclose(r["H"], Ho, rtol=0, atol=1e-10 * max(np.abs(Ho).max(), 1e-300))
    assert np.allclose(r["b"], bo, rtol=0, atol=1e-10 * max(1.0, np.abs(bo).max()))
    with capsys.disabled():
        print("\n[%s]" % name)
        ref, ratio, x1 = check_step(r["H"], r["b"], r["X_iters"][0], r["X"])
    if name == "one plane":
        assert ref["live"] == (2, 3, 4)
        assert r["X"][9] == s.T0[0, 3] and r["X"][10] == s.T0[1, 3]           # x, y ...
        assert r["X"][1] == 0.0 and r["X"][3] == 0.0                        # ... and yaw: bit for bit those of X0
    if name == "no matches":
        assert np.array_equal(r["X"], O.pose12(s.T0)) and not r["H"].any() and not r["b"].any() and not r["matched"].any()


def test_scenes_are_in_their_regimes_on_the_device(ctx, scenes):
    """The conditions tests/test_gn_step_ref.py shows for the oracle's H, b, asserted again from the device's own: a scene that
    drifts out of its regime fails here instead of silently testing something else."""
    refs, lins = {}, {}
    for name in G.CASES:
        s = scenes(name)
        r = register(ctx, s, 1)
        refs[name] = G.step(r["H"], r["b"], r["X_iters"][0])
        lins[name] = dict(H=r["H"], b=r["b"], matched=r["matched"], abs_e=G.oracle_linearize(name)["abs_e"])
    orders = G.check_conditions(refs, lins)
    assert len(orders) >= 6
    assert {refs[n]["branch"] for n in G.CASES} == {"first-order", "sin_small", "libm"}


@pytest.mark.parametrize("n_iters", [1, 2, 15])
def test_no_matches_leaves_everything_untouched(ctx, scenes, n_iters):
    s = scenes("no matches")
    X0 = O.pose12(s.T0)
    r = register(ctx, s, n_iters)
    assert np.array_equal(r["X"], X0)
    assert np.array_equal(r["X_iters"], np.tile(X0, (n_iters, 1)))
    assert not r["H"].any() and not r["b"].any()
    assert not r["matched"].any() and int(r["matched"].sum()) == 0
    bat = ctx.icp_register_batch([s.mid], [s.tid], X0[None, :], s.params, n_iters)
    assert np.array_equal(bat["X"][0], X0) and not bat["H"].any() and not bat["b"].any() and bat["n_matched"][0] == 0


@pytest.mark.parametrize("name", LATER)
def test_later_rounds(ctx, scenes, name, capsys):
    """n_iters = 1 .. 6: (a) the poses are the first rows of the 15-round run, bit for bit — registration is deterministic and
    the join order does not depend on the round count; both parities of the pose ring and of the double-buffered partials;
    (b) the last step of every run against the exact solve of that run's H, b; (c) at the oracle's poses of rounds 0, 1 and
    5, injected, the device's correspondences and gate bits are the oracle's."""
    s = scenes(name)
    full = register(ctx, s, 15)
    poses = np.concatenate([full["X_iters"], full["X"][None, :]])
    branches, orders = set(), set()
    with capsys.disabled():
        print("\n[%s, later rounds]" % name)
        for r in range(1, 7):
            run = register(ctx, s, r)
            assert np.array_equal(run["X_iters"], poses[:r]), r
            assert np.array_equal(run["X"], poses[r]), r
            ref, _, _ = check_step(run["H"], run["b"], run["X_iters"][r - 1], run["X"], later=r > 1)
            branches.add(ref["branch"])
            orders.add(ref["order"])
    assert "first-order" in branches and len(branches) >= 2
    # the first-order branch's I + skew(w) is no rotation (its singular values are sqrt(1 + |w|^2)), so R leaves the rotations
    # by up to 5e-9 a round BY THE FORMULA — why recover() inverts R0 instead of transposing it — and moved[]'s use assumes
    # |R|_2 <= 1 + 1e-7 after 15 updates (kernels.hip.h, above solve_pose): held here on every pose of the run
    for X in poses:
        assert np.linalg.norm(X[:9].reshape(3, 3), 2) <= 1.0 + 1e-7
    o = O.icp_register(s.om, [s.of], s.T0, 15, *s.params)
    for r in (0, 1, 5):
        check_inputs_at(ctx, s, O.pose44(o["X_iters"][r]))
    d = np.linalg.inv(o["T"]) @ full["T"]
    assert np.linalg.norm(d[:3, 3]) <= 1e-5 and np.abs(d[:3, :3] - np.eye(3)).max() <= 1e-5


@pytest.mark.parametrize("name", ["large step", "lever arm"])
def test_reuse_is_exact_under_large_steps(ctx, scenes, name):
    """tests/test_gpu_parity.py::test_correspondence_reuse_is_exact under steps where moved[] is large (0.66 rad; 1 m at a 300 m
    lever arm): a moved[] that under-reported them would let a stale pair or gate decision through."""
    s = scenes(name)
    res = {}
    try:
        for tag, opts in (("on", dict()), ("no reuse", dict(cache_correspondences=0)), ("no gate reuse", dict(cache_gate=0))):
            for k, v in opts.items():
                ctx.set_option(k, v)
            res[tag] = register(ctx, s, 15)
            for k in opts:
                ctx.set_option(k, 1)
    finally:
        ctx.set_option("cache_correspondences", 1)
        ctx.set_option("cache_gate", 1)
    steps = np.abs(np.diff(res["on"]["X_iters"], axis=0)).max(axis=1)
    assert steps[0] > 0.04          # (the first step is a large one: that is the point)
    for tag in ("no reuse", "no gate reuse"):
        for key in KEYS:
            assert np.array_equal(res["on"][key], res[tag][key]), (tag, key)
        assert res["on"]["visits"] == res[tag]["visits"], tag


@pytest.mark.parametrize("option", ["persistent", "xcd_fold"])
def test_all_three_call_sites(ctx, scenes, option):
    """solve_pose is called from the prologue of icp_round, the loop of icp_persist and icp_final: every scene gives the bits
    of the default route under either option."""
    assert ctx.get_option(option) == 0
    runs = [(name, n) for name in G.CASES for n in ((1,) if name in SINGLE_ROUND else (1, 2, 5))]
    res = {}
    try:
        for on in (0, 1):
            ctx.set_option(option, on)
            res[on] = [register(ctx, scenes(name), n) for name, n in runs]
    finally:
        ctx.set_option(option, 0)
    for (name, n), a, b in zip(runs, res[0], res[1]):
        for key in KEYS:
            assert np.array_equal(a[key], b[key]), (name, n, key)
        assert a["visits"] == b["visits"], (name, n)


def test_batch_isolation(ctx, scenes):
    """One batch of [no matches, mid step, one plane, mid step again] against one tree list (the mid-step corner and the plane,
    100 m apart) and one parameter set: a row's solve sees nothing of its neighbours'."""
    shift = np.array([100.0, 100.0, 0.0])
    plane = G.case("one plane")
    hp = capi.HostTree(plane["fixed"] + shift, G.TREE_B_MAX, G.TREE_B_MIN, 2)
    hq = capi.HostTree(plane["moving"] + shift, G.TREE_B_MAX, G.TREE_B_MIN, 2)
    mid_s, none_s = scenes("mid step"), scenes("no matches")
    tids = [mid_s.tid, ctx.tree_upload(hp.nodes, hp.num_leaves)]
    clouds = [none_s.moving_leaves, mid_s.moving_leaves, hq.leaf_means(), mid_s.moving_leaves]
    T0s = [none_s.T0, mid_s.T0, plane["T0"], mid_s.T0]
    mids = [ctx.moving_upload(c) for c in clouds]
    X0 = np.stack([capi.pose12(T) for T in T0s])
    try:
        bat = ctx.icp_register_batch(mids, tids, X0, G.DEFAULT, 1)
        flags = [ctx.icp_fetch_matched(i, c.shape[0]) for i, c in enumerate(clouds)]
        alone = [ctx.icp_register(m, tids, T, G.DEFAULT, 1, c.shape[0]) for m, T, c in zip(mids, T0s, clouds)]
    finally:
        ctx.tree_release(tids[1])
        for m in mids:
            ctx.moving_release(m)
    assert np.isfinite(bat["X"]).all() and np.isfinite(bat["H"]).all() and np.isfinite(bat["b"]).all()
    for key in ("X", "H", "b", "n_matched", "visits"):
        assert np.array_equal(bat[key][1], bat[key][3]), key
    assert np.array_equal(flags[1], flags[3]) and bat["n_matched"][1] > 50          # (a real row: pairs, a solve, a step)
    assert np.abs(bat["X"][1] - X0[1]).max() > 1e-3
    assert np.array_equal(bat["X"][0], X0[0]) and not bat["H"][0].any() and not bat["b"][0].any()
    assert bat["n_matched"][0] == 0 and not flags[0].any()
    Hp = bat["H"][2]
    assert bat["n_matched"][2] > 1000 and not Hp[[0, 1, 5], :].any() and not Hp[:, [0, 1, 5]].any()
    assert bat["X"][2][9] == 0.0 and bat["X"][2][10] == 0.0 and bat["X"][2][1] == 0.0 and bat["X"][2][3] == 0.0
    for i, a in enumerate(alone):
        assert np.allclose(bat["X"][i], a["X"], rtol=0, atol=1e-10), i
        assert np.allclose(bat["H"][i], a["H"], rtol=0, atol=1e-10 * max(np.abs(a["H"]).max(), 1e-300)), i
        assert np.allclose(bat["b"][i], a["b"], rtol=0, atol=1e-10 * max(1.0, np.abs(a["b"]).max())), i
        assert np.array_equal(flags[i], a["matched"]) and bat["n_matched"][i] == int(a["matched"].sum()), i
