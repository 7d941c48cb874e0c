"""One Gauss-Newton update `X0, H, b -> X1` (MADicp::updateState, mad_icp.cpp:105-117) in high precision, and the small
scenes that drive the device's update step (solve_pose in mad_icp_amd/csrc/hip/kernels.hip.h) to its edges.

TEST INFRASTRUCTURE ONLY (a helper like descent_ref.py).  `step` takes the doubles a registration returns — the joined 6x6 H
(its lower triangle is mirrored), b, and the pose before the round as 12 doubles — and computes, with mpmath at PREC bits:

  dx      the exact solution of H dx = -b for those doubles.  A row (and column) of H that is exactly zero gives dx_i = 0 and
          the remaining block is solved: what Eigen's LDLT returns for such a matrix and what both device solvers claim.
  X1      the pose after the update by the REFERENCE's formula, lie_algebra.h:39-52 — not the true exponential:
          dR = I + skew(w) below |w|^2 < 1e-8, Rodrigues' I + sin(th) K + 2 sin^2(th/2) K^2 from there on; R1 = R0 dR,
          t1 = R0 dx_t + t0 (mad_icp.cpp:114-116).
  kappa_s the 2-norm condition number of D^-1 H D^-1, D = sqrt(diag H), on the block that is solved; kappa that of H itself.
  order   the pivot order of Eigen::LDLT on this H: the diagonal sorted by decreasing magnitude, ties to the lower index.
  branch  which way the device's exp_so3 goes: "first-order" (|w|^2 < 1e-8), "sin_small" (|w| <= 0.5), "libm".

`err` is the error measure of a computed dx, |D (dx - dx_exact)| / |D dx_exact|, and `recover` inverts the composition: the
dx that takes X0 to a given X1.  tests/test_gn_step_ref.py holds all of it to the oracle's double LDLT and expMapSO3."""
import functools

import mpmath as mp
import numpy as np

PREC = 256
U = 2.0 ** -53  # unit roundoff of a double


def _mat(a, r, c):
    a = np.asarray(a, dtype=np.float64).reshape(r, c)
    return mp.matrix([[mp.mpf(float(a[i, j])) for j in range(c)] for i in range(r)])


def sym(H):
    """the 6x6 as the solvers read it: the lower triangle, mirrored"""
    H = np.asarray(H, dtype=np.float64).reshape(6, 6)
    return np.tril(H) + np.tril(H, -1).T


def pivot_order(H):
    d = np.abs(np.diag(np.asarray(H, dtype=np.float64).reshape(6, 6)))
    return tuple(sorted(range(6), key=lambda i: (-d[i], i)))


def _cond(M):
    ev = [abs(x) for x in mp.eigsy(M, eigvals_only=True)]
    return max(ev) / min(ev)


def _skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def exp_ref(w):
    """lie_algebra.h:39-52 on mpf"""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    W = _skew(w)
    if th2 < mp.mpf("1e-8"):
        return mp.eye(3) + W
    th = mp.sqrt(th2)
    K = W / th
    return mp.eye(3) + mp.sin(th) * K + 2 * mp.sin(th / 2) ** 2 * (K * K)


def step(H, b, X0):
    with mp.workprec(PREC):
        Hs = sym(H)
        bb = np.asarray(b, dtype=np.float64).reshape(6)
        X0 = np.asarray(X0, dtype=np.float64).reshape(12)
        live = [i for i in range(6) if np.any(Hs[i] != 0.0)]
        dx = [mp.mpf(0)] * 6
        kappa_s = kappa = mp.mpf(1)
        if live:
            n = len(live)
            A = mp.matrix(n, n)
            for a_, i in enumerate(live):
                for c_, j in enumerate(live):
                    A[a_, c_] = mp.mpf(float(Hs[i, j]))
            sol = mp.lu_solve(A, mp.matrix([-mp.mpf(float(bb[i])) for i in live]))
            for a_, i in enumerate(live):
                dx[i] = sol[a_]
            S = mp.matrix(n, n)
            for a_ in range(n):
                for c_ in range(n):
                    S[a_, c_] = A[a_, c_] / mp.sqrt(A[a_, a_] * A[c_, c_])
            kappa_s, kappa = _cond(S), _cond(A)
        w = dx[3:]
        th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        th = mp.sqrt(th2)
        branch = "first-order" if th2 < mp.mpf("1e-8") else ("sin_small" if th <= mp.mpf("0.5") else "libm")
        R0, t0 = _mat(X0[:9], 3, 3), _mat(X0[9:], 3, 1)
        R1 = R0 * exp_ref(w)
        t1 = R0 * mp.matrix(dx[:3]) + t0
        X1 = [R1[i, j] for i in range(3) for j in range(3)] + [t1[i] for i in range(3)]
        return dict(dx=dx, X1=X1, dx64=np.array([float(v) for v in dx]), X164=np.array([float(v) for v in X1]),
                    kappa_s=float(kappa_s), kappa=float(kappa), order=pivot_order(Hs), branch=branch, theta=float(th),
                    theta2=float(th2), live=tuple(live), D=np.sqrt(np.abs(np.diag(Hs))))


def err(ref, dx):
    """|D (dx - dx_exact)| / |D dx_exact| of a computed dx (doubles or mpf) against step()'s result; 0 for 0 against 0."""
    with mp.workprec(PREC):
        D = [mp.sqrt(mp.mpf(float(d)) ** 2) for d in ref["D"]]
        num = mp.sqrt(sum((D[i] * (mp.mpf(dx[i]) - ref["dx"][i])) ** 2 for i in range(6)))
        den = mp.sqrt(sum((D[i] * ref["dx"][i]) ** 2 for i in range(6)))
        if den == 0:
            return 0.0 if num == 0 else float("inf")
        return float(num / den)


def recover(X0, X1, first_order):
    """The dx (six mpf) that takes X0 to X1: dx_t = R0^-1 (t1 - t0), and dx_w from dR = R0^-1 R1 — the skew part of dR - I
    where the update took the first-order branch, the logarithm of dR otherwise.  R0^-1 is R0' for a rotation; the inverse is
    what undoes the composition for the doubles R0 really holds (orthogonal to rounding only)."""
    with mp.workprec(PREC):
        X0 = np.asarray(X0, dtype=np.float64).reshape(12)
        X1 = np.asarray(X1, dtype=np.float64).reshape(12)
        Ri = _mat(X0[:9], 3, 3) ** -1
        dt = Ri * (_mat(X1[9:], 3, 1) - _mat(X0[9:], 3, 1))
        dR = Ri * _mat(X1[:9], 3, 3)
        v = [(dR[2, 1] - dR[1, 2]) / 2, (dR[0, 2] - dR[2, 0]) / 2, (dR[1, 0] - dR[0, 1]) / 2]  # sin(th) k
        if not first_order:
            s = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
            c = (dR[0, 0] + dR[1, 1] + dR[2, 2] - 1) / 2
            if s != 0:
                th = mp.atan2(s, c)
                v = [th * x / s for x in v]
        return [dt[0], dt[1], dt[2], v[0], v[1], v[2]]


def composition_slack(X0):
    """4 u (1 + |t0|): what the double composition R0 dR, R0 dx_t + t0 may add to an entry of X1 (three products and three
    sums of terms bounded by 1, by |t0| + |dx_t| for the translation) on top of the solver's error."""
    X0 = np.asarray(X0, dtype=np.float64).reshape(12)
    return 4.0 * U * (1.0 + float(np.linalg.norm(X0[9:])))


def bounds(ref, X0, c):
    """-> (beta, dx_slack, x1_tol).  beta = c kappa_s u bounds err(dx).  A dx RECOVERED from a pose in doubles also carries that
    pose's composition rounding: composition_slack per entry of X1, at most doubled by R0^-1 (row sums of a rotation are at
    most sqrt 3) — dx_slack is that, in the measure of err.  x1_tol (12,) is beta propagated to the entries of X1 —
    |d dx_i| <= beta |D dx| / D_i; |d t1| <= |d dx_t|, |d R1_ij| <= |d w| (the derivative of the exponential has norm one, a
    rotation's rows have norm one) — plus the composition slack."""
    beta = c * ref["kappa_s"] * U
    D = ref["D"]
    comp = composition_slack(X0)
    Ddx = float(np.linalg.norm(D * ref["dx64"]))
    dx_slack = 2.0 * comp * float(np.linalg.norm(D)) / Ddx if Ddx > 0 else 0.0
    ddx = np.array([beta * Ddx / D[i] if D[i] > 0 else 0.0 for i in range(6)])
    x1_tol = np.concatenate([np.full(9, np.linalg.norm(ddx[3:])), np.full(3, np.linalg.norm(ddx[:3]))]) + comp
    return beta, dx_slack, x1_tol


# ---- the scenes --------------------------------------------------------------------------------------------------------------

TREE_B_MAX, TREE_B_MIN = 0.2, 0.1
OPEN = (50.0, 100.0, 1.0)        # (min_ball, rho_ker, b_ratio): every pair accepted, no Huber damping
DEFAULT = (0.2, 0.1, 0.02)       # mad_icp/configurations/default.cfg


def corner(n, s, seed=5):
    """Three mutually orthogonal square faces of side s meeting at the origin, n uniform points each, the face coordinate
    exactly 0.0."""
    rng = np.random.default_rng(seed)
    faces = []
    for axis in range(3):
        p = rng.uniform(0.0, s, (n, 3))
        p[:, axis] = 0.0
        faces.append(p)
    return np.concatenate(faces)


def rot_x(a):
    T = np.eye(4)
    c, s = np.cos(a), np.sin(a)
    T[1:3, 1:3] = [[c, -s], [s, c]]
    return T


def _case(fixed, moving, T0, params):
    return dict(fixed=np.ascontiguousarray(fixed), moving=np.ascontiguousarray(moving), T0=T0, params=params)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(fixed (N,3), moving (M,3), T0 (4,4), params).  The fixed tree holds all points, the moving cloud is every second
    one; T0 is a rotation about x unless the case says otherwise."""
    if name == "large step":
        c = corner(1500, 0.6)
        return _case(c, c[::2], rot_x(0.6), OPEN)
    if name == "mid step":
        c = corner(1500, 2.0)
        return _case(c, c[::2], rot_x(0.3), OPEN)
    if name == "first-order":
        c = corner(1500, 20.0)
        T0 = np.eye(4)
        T0[0, 3] = 1e-3
        return _case(c, c[::2], T0, OPEN)
    if name == "big room":
        c = corner(1500, 80.0)
        return _case(c, c[::2], rot_x(0.3), OPEN)
    if name == "lever arm":
        # the corner stands 300 m from the sensor origin in the moving frame; T0 = rot_x(0.05) about the corner, so it brings
        # the cloud back onto the fixed one up to that rotation
        c = corner(1500, 2.0)
        off = np.array([300.0, 0.0, 0.0])
        T0 = rot_x(0.05)
        T0[:3, 3] = -T0[:3, :3] @ off
        return _case(c, c[::2] + off, T0, OPEN)
    if name == "Huber-dominant":
        # 0.5 m along EVERY face normal: every pair's |e| is 0.5, above sqrt(rho_ker) = 0.32 where the kernel damps
        c = corner(1500, 20.0)
        T0 = np.eye(4)
        T0[:3, 3] = 0.5
        return _case(c, c[::2], T0, (50.0, 0.1, 1.0))
    if name == "Huber one face":
        # 0.5 m along ONE face normal: the pairs of that face (a third of all) are damped, the others are not
        c = corner(1500, 20.0)
        T0 = np.eye(4)
        T0[0, 3] = 0.5
        return _case(c, c[::2], T0, (50.0, 0.1, 1.0))
    if name == "diagonal tie":
        # two congruent faces, x = 0 and y = 0 (the same (u, v) on both), a pure translation, no damping, and a min_ball of 1e6:
        # a leaf's weight (1 - bbox0 / min_ball)^2 is exactly 1 even where the builder left an extent of 1e-12 on a flat leaf, so
        # H_00 and H_11 are the same INTEGER — the pair count of a face, exact in any summation order — and row 2 is exactly zero
        uv = np.random.default_rng(8).uniform(0.0, 4.0, (2000, 2))
        z = np.zeros(2000)
        c = np.concatenate([np.stack([z, uv[:, 0], uv[:, 1]], 1), np.stack([uv[:, 0], z, uv[:, 1]], 1)])
        T0 = np.eye(4)
        T0[:3, 3] = [0.02, 0.01, 0.0]
        return _case(c, c[::2], T0, (1.0e6, 100.0, 1.0))
    if name == "one plane":
        rng = np.random.default_rng(6)
        p = rng.uniform(0.0, 10.0, (4000, 3))
        p[:, 2] = 0.0
        T0 = np.eye(4)
        T0[2, 3] = 0.03
        return _case(p, p[::2], T0, DEFAULT)
    if name == "no matches":
        c = corner(1500, 10.0)
        T0 = np.eye(4)
        T0[0, 3] = 200.0
        return _case(c, c[::2], T0, DEFAULT)
    raise KeyError(name)


CASES = ("large step", "mid step", "first-order", "big room", "lever arm", "Huber-dominant", "Huber one face", "one plane",
         "no matches", "diagonal tie")


# ---- the oracle on the scenes (CPU): what tests/test_gn_step_ref.py measures and tests/test_gpu_gn_step.py takes its c from -----

@functools.lru_cache(maxsize=None)
def oracle_trees(name):
    """-> (fixed, moving) oracle trees of a case"""
    import oracle_lib as O

    cs = case(name)
    return O.Tree(cs["fixed"], TREE_B_MAX, TREE_B_MIN, 2), O.Tree(cs["moving"], TREE_B_MAX, TREE_B_MIN, 2)


def oracle_linearize(name, T=None):
    """One MADicp::update of the case at pose T (default: its T0) -> dict(H, b, corr, rej, matched, depth, abs_e): abs_e is
    |e| of the accepted pairs, e = (T p - f.mean) . f.normal (mad_icp.cpp:85)."""
    import oracle_lib as O

    cs = case(name)
    ft, mt = oracle_trees(name)
    T = cs["T0"] if T is None else np.asarray(T, dtype=np.float64)
    H, b, corr, rej, mat, depth = O.icp_linearize(mt, ft, T, *cs["params"])
    fm, fn, _ = ft.leaves()
    ml = mt.leaves()[0] @ T[:3, :3].T + T[:3, 3]
    e = np.abs(((ml - fm[corr]) * fn[corr]).sum(axis=1))[rej == 0]
    return dict(H=sym(H), b=b, corr=corr, rej=rej, matched=mat, depth=depth, abs_e=e)


@functools.lru_cache(maxsize=None)
def oracle_ratio(name):
    """err(dx_oracle) / (kappa_s u) of the case's first round: the oracle's double LDLT against the exact solve of the same H, b"""
    import oracle_lib as O

    lin = oracle_linearize(name)
    ref = step(lin["H"], lin["b"], O.pose12(case(name)["T0"]))
    return err(ref, O.ldlt6_solve(lin["H"], -lin["b"])) / (ref["kappa_s"] * U)


@functools.lru_cache(maxsize=None)
def rho_ref():
    """The reference's own error ratio: the largest oracle_ratio over the cases.  The device's bound is c = 8 rho_ref."""
    return max(oracle_ratio(name) for name in CASES)


def check_conditions(refs, lins):
    """Every scene is in the regime it is there for.  refs: name -> step() of the first round's H, b; lins: name -> dict(H, b,
    matched, abs_e) of that round (abs_e: |e| of the accepted pairs, from the oracle).  Asserted on the oracle's H, b by
    tests/test_gn_step_ref.py and again on the device's own by tests/test_gpu_gn_step.py."""
    r = refs["large step"]
    assert r["theta"] > 0.5 and r["branch"] == "libm", r["theta"]
    assert r["order"][0] in (0, 1, 2), r["order"]                      # a translation diagonal leads
    r = refs["mid step"]
    assert 1e-4 < r["theta"] <= 0.5 and r["branch"] == "sin_small", r["theta"]
    assert set(r["order"][:3]) == {3, 4, 5}, r["order"]                # the rotation diagonals lead
    r = refs["first-order"]
    assert r["theta2"] < 1e-8 and abs(r["theta2"] / 1e-8 - 1.0) > 1e-3 and r["branch"] == "first-order", r["theta2"]
    assert r["theta"] > 0.0
    assert refs["big room"]["kappa"] >= 1e3, refs["big room"]["kappa"]
    assert refs["lever arm"]["kappa_s"] >= 1e4, refs["lever arm"]["kappa_s"]
    for name in CASES:
        if name not in ("lever arm", "no matches"):
            assert refs[name]["kappa_s"] < 100.0, (name, refs[name]["kappa_s"])   # (the other scenes are well conditioned)
    rho_ker = case("Huber-dominant")["params"][1]
    e = lins["Huber-dominant"]["abs_e"]
    assert e.size > 1000 and (e > np.sqrt(rho_ker)).mean() > 0.5        # damped where the kernel damps: chi > sqrt(rho_ker)
    assert (e > rho_ker).mean() > 0.5
    e = lins["Huber one face"]["abs_e"]
    assert 0.3 < (e > np.sqrt(rho_ker)).mean() < 0.5                    # one face of three
    H = lins["one plane"]["H"]
    assert not H[[0, 1, 5], :].any() and not H[:, [0, 1, 5]].any() and refs["one plane"]["live"] == (2, 3, 4)
    assert lins["one plane"]["matched"].sum() > 1000
    normals = oracle_trees("one plane")[0].leaves()[1]
    assert np.array_equal(np.abs(normals), np.tile([0.0, 0.0, 1.0], (normals.shape[0], 1)))
    n = lins["no matches"]
    assert not n["H"].any() and not n["b"].any() and n["matched"].sum() == 0 and refs["no matches"]["live"] == ()
    H, o = lins["diagonal tie"]["H"], refs["diagonal tie"]["order"]
    assert H[0, 0] == H[1, 1] and H[0, 0] >= 100.0                      # an exact tie of two non-zero diagonal entries ...
    assert o.index(1) == o.index(0) + 1                                 # ... that Eigen's order gives to the lower index
    assert not H[2, :].any() and refs["diagonal tie"]["live"] == (0, 1, 3, 4, 5)
    orders = {refs[name]["order"] for name in CASES}
    assert len(orders) >= 6, orders
    return orders
