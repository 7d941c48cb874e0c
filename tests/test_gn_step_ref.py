"""tests/gn_step_ref.py held to the oracle (no GPU), and the conditions of the scenes of tests/test_gpu_gn_step.py shown to hold
before any GPU run.

The high-precision update `X0, H, b -> X1` is compared with the oracle's own double arithmetic — oracle_lib.ldlt6_solve
(Eigen::LDLT's algorithm), oracle_lib.expmap_so3 (lie_algebra.h:39-52) and a plain double composition — on H, b of
oracle_lib.icp_linearize for every scene; that is what makes it a reference and not a third opinion.  The same comparison
measures the reference's own error ratio

    rho_ref = max over the scenes of  err(dx_oracle) / (kappa_s 2^-53),    err(dx) = |D (dx - dx_exact)| / |D dx_exact|,

which is what the device's bound is made of (c = 8 rho_ref, tests/test_gpu_gn_step.py).  Measured here: 0.11 ... 0.50 per
scene (largest on "Huber one face"), so rho_ref = 0.50 and c = 4.0.

The product's host library takes the same exam (capi.gn_update, MADicp::updateState of mad_icp_amd/csrc/host): first rounds and
the rounds that follow.  Its figures show what a recovered dx can be asked: at the first round of every scene the dx recovered
from its X1 meets c kappa_s 2^-53 as it stands; from the fourth round on the steps are 1e-7 and smaller, the double
composition t1 = R0 dx_t + t0 alone rounds at 1e-16, and the recovered dx of this double-precision update is off by up to
1e-5 of itself ("later rounds" below) — the allowance gn_step_ref.bounds adds for that is the composition's own rounding,
nothing else, and the entries of X1 are held to the propagated bound in every round."""
import mpmath as mp
import numpy as np
import pytest

import gn_step_ref as G
import oracle_lib as O
from mad_icp_amd import capi

LATER = ("large step", "lever arm", "Huber-dominant")


def oracle_update(H, b, X0):
    """the oracle's double update, piece by piece: LDLT, expMapSO3, compose"""
    dx = O.ldlt6_solve(H, -b)
    R0, t0 = X0[:9].reshape(3, 3), X0[9:]
    return dx, np.concatenate([(R0 @ O.expmap_so3(dx[3:])).reshape(-1), R0 @ dx[:3] + t0])


@pytest.mark.parametrize("name", G.CASES)
def test_reference_agrees_with_the_oracles_double_update(name, capsys):
    cs, lin = G.case(name), G.oracle_linearize(name)
    X0 = O.pose12(cs["T0"])
    ref = G.step(lin["H"], lin["b"], X0)
    dx_o, X1_o = oracle_update(lin["H"], lin["b"], X0)
    ratio = G.err(ref, dx_o) / (ref["kappa_s"] * G.U)
    assert ratio == pytest.approx(G.oracle_ratio(name))
    assert ratio <= 1.0                                       # (a backward-stable solve: well inside kappa_s u)
    c = 8.0 * G.rho_ref()
    beta, slack, x1_tol = G.bounds(ref, X0, c)
    assert (np.abs(X1_o - ref["X164"]) <= x1_tol).all()
    # the dead rows: Eigen's LDLT gives exactly zero there
    dead = [i for i in range(6) if i not in ref["live"]]
    assert all(dx_o[i] == 0.0 for i in dead) and all(ref["dx"][i] == 0 for i in dead)
    # recover() undoes the composition: from the oracle's X1, and from the product's host update, at the bound as it stands
    first = ref["branch"] == "first-order"
    X1_h = capi.gn_update(lin["H"], lin["b"], X0)
    e_o, e_h = G.err(ref, G.recover(X0, X1_o, first)), G.err(ref, G.recover(X0, X1_h, first))
    with capsys.disabled():
        print("\n[%s] order %s, %s (|w| = %.3g), kappa_s %.3g, cond(H) %.3g, oracle ratio %.3f; recovered: oracle %.3g, host "
              "%.3g of the bound" % (name, ref["order"], ref["branch"], ref["theta"], ref["kappa_s"], ref["kappa"], ratio,
                                     e_o / beta, e_h / beta))
    assert e_o <= beta and e_h <= beta
    assert (np.abs(X1_h - ref["X164"]) <= x1_tol).all()


def test_rho_ref(capsys):
    per = {name: G.oracle_ratio(name) for name in G.CASES}
    with capsys.disabled():
        print("\n[rho_ref] " + ", ".join("%s %.3f" % kv for kv in per.items()) + " -> rho_ref %.3f, c = %.2f"
              % (G.rho_ref(), 8.0 * G.rho_ref()))
    assert G.rho_ref() == max(per.values())
    live = [v for k, v in per.items() if k != "no matches"]
    assert min(live) >= 0.02 and G.rho_ref() <= 1.0     # every scene measures something; none is outside kappa_s u


def test_every_scene_meets_its_condition():
    refs, lins = {}, {}
    for name in G.CASES:
        lins[name] = G.oracle_linearize(name)
        refs[name] = G.step(lins[name]["H"], lins[name]["b"], O.pose12(G.case(name)["T0"]))
    G.check_conditions(refs, lins)


def test_check_conditions_notices_a_scene_out_of_its_regime():
    refs, lins = {}, {}
    for name in G.CASES:
        lins[name] = G.oracle_linearize(name)
        refs[name] = G.step(lins[name]["H"], lins[name]["b"], O.pose12(G.case(name)["T0"]))
    for a, b in (("large step", "mid step"), ("first-order", "mid step"), ("lever arm", "mid step"), ("one plane", "mid step"),
                 ("Huber-dominant", "Huber one face"), ("diagonal tie", "big room")):
        swapped = dict(refs, **{a: refs[b]})
        swapped_l = dict(lins, **{a: lins[b]})
        with pytest.raises(AssertionError):
            G.check_conditions(swapped, swapped_l)


@pytest.mark.parametrize("name", LATER)
def test_later_rounds(name, capsys):
    """Rounds 0..6 of the oracle's registration: the reference follows the oracle's poses, the pivot orders and branches
    change on the way, and the host's double update meets the bound with the composition's allowance — and, printed, how far
    over the bare bound the recovered dx of that double update is once the steps are tiny."""
    cs = G.case(name)
    ft, mt = G.oracle_trees(name)
    o = O.icp_register(mt, [ft], cs["T0"], 15, *cs["params"])
    c = 8.0 * G.rho_ref()
    lines, branches = [], set()
    for r in range(7):
        X0 = o["X_iters"][r]
        lin = G.oracle_linearize(name, O.pose44(X0))
        ref = G.step(lin["H"], lin["b"], X0)
        beta, slack, x1_tol = G.bounds(ref, X0, c)
        assert (np.abs(o["X_iters"][r + 1] - ref["X164"]) <= x1_tol).all(), r      # the oracle's next pose
        X1_h = capi.gn_update(lin["H"], lin["b"], X0)
        assert (np.abs(X1_h - ref["X164"]) <= x1_tol).all(), r
        e_h = G.err(ref, G.recover(X0, X1_h, ref["branch"] == "first-order"))
        assert e_h <= beta + slack, (r, e_h, beta, slack)
        branches.add(ref["branch"])
        lines.append("r%d %s |w| %.2g: recovered %.2g x bound, allowance %.2g x" % (r, ref["branch"], ref["theta"], e_h / beta,
                                                                                  slack / beta))
    with capsys.disabled():
        print("\n[%s] " % name + "; ".join(lines))
    assert "first-order" in branches and "sin_small" in branches


def test_zero_rows_are_left_out_and_the_rest_is_solved():
    rng = np.random.default_rng(1)
    A = rng.normal(size=(8, 6))
    H = A.T @ A
    b = rng.normal(size=6)
    for dead in ((), (0,), (5,), (0, 1, 5), (1, 2, 3, 4), (0, 1, 2, 3, 4, 5)):
        Hd, live = H.copy(), [i for i in range(6) if i not in dead]
        Hd[list(dead), :] = 0.0
        Hd[:, list(dead)] = 0.0
        ref = G.step(Hd, b, O.pose12(np.eye(4)))
        assert ref["live"] == tuple(live)
        want = np.zeros(6)
        if live:
            want[live] = np.linalg.solve(Hd[np.ix_(live, live)], -b[live])
        assert np.allclose(ref["dx64"], want, rtol=1e-10, atol=0)
        assert all(ref["dx"][i] == 0 for i in dead)
        assert np.allclose(O.ldlt6_solve(Hd, -b), want, rtol=1e-10, atol=0)   # (what Eigen's LDLT does, as the oracle restates it)
        if live:
            S = Hd[np.ix_(live, live)] / np.sqrt(np.outer(np.diag(Hd)[live], np.diag(Hd)[live]))
            assert ref["kappa_s"] == pytest.approx(np.linalg.cond(S), rel=1e-9)
            assert ref["kappa"] == pytest.approx(np.linalg.cond(Hd[np.ix_(live, live)]), rel=1e-9)


def test_pivot_order_and_ties():
    assert G.pivot_order(np.diag([3.0, 5.0, 1.0, 5.0, -7.0, 0.0])) == (4, 1, 3, 0, 2, 5)
    assert G.pivot_order(np.zeros((6, 6))) == (0, 1, 2, 3, 4, 5)
    assert G.sym(np.tril(np.arange(36.0).reshape(6, 6)))[1, 4] == 25.0      # only the lower triangle is read


def test_rotation_follows_the_reference_formula_on_both_sides_of_its_threshold():
    for th, first in ((0.99e-4, True), (1.01e-4, False), (0.3, False), (0.7, False), (1.2, False)):
        w = th * np.array([0.6, -0.48, 0.64])
        with mp.workprec(G.PREC):
            R = G.exp_ref([mp.mpf(float(x)) for x in w])
            R64 = np.array([[float(R[i, j]) for j in range(3)] for i in range(3)])
            assert (R[0, 0] == 1) == first      # first order: I + skew(w), a diagonal of exactly one
        assert np.abs(R64 - O.expmap_so3(w)).max() <= 4 * G.U
        X1 = np.concatenate([R64.reshape(-1), [0.1, 0.2, 0.3]])
        rec = G.recover(O.pose12(np.eye(4)), X1, first)
        assert np.allclose([float(x) for x in rec[3:]], w, rtol=0, atol=8 * G.U)  # (R64 is rounded: half an ulp of 1 an entry)
        assert [float(x) for x in rec[:3]] == [0.1, 0.2, 0.3]
    # below the threshold the formula is NOT the exponential: the two differ by th^2 / 2, far above any tolerance used here
    w = np.array([0.9e-4, 0.0, 0.0])
    with mp.workprec(G.PREC):
        R = G.exp_ref([mp.mpf(float(x)) for x in w])
        assert abs(float(R[1, 1] - mp.cos(mp.mpf(float(w[0]))))) > 1e-9
