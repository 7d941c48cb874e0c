"""An EXACT reference for the surfel of a voxel-map row (mad_icp_amd/csrc/common/voxel_moments.h: map_surfel) that contains no
eigen-solver, and the catalogue of voxel populations the host and the device tests share.  Standard library and numpy only.

From a row's ten words (n | S1[3] | S2[6]) the integer matrix A = n S2 - S1 S1^T is formed in Python integers: A = n^2 C exactly,
where C is the covariance of the offsets in offset units squared.  Everything below is in C's units unless it says otherwise; an
eigenvalue in m^2 is that times s^2, s = voxel / 65536.
  rank          0 .. 3, from integer minors
  spectrum      the three eigenvalues, each BRACKETED by bisection in integers: the number of eigenvalues of A below x is the number
                of sign changes in (1, t, m, d), the invariants of A - x I (Descartes' rule, exact for a polynomial whose roots are
                all real); an eigenvalue the rank says is zero is the bracket [0, 0]
  certificate   for a claimed pair (float32 eigenvalue, float32 vector), in fractions.Fraction: r = C v - lambda' v; ||r|| / ||v||
                and ||v||^2.  Weyl: an exact eigenvalue lies within ||r|| / ||v|| of lambda'.  Davis-Kahan: the sine of the angle
                to the exact eigenspace is at most (||r|| / ||v||) / gap, gap = the distance of lambda' to the OTHER exact eigenvalues
  eigenvector   of a bracketed simple eigenvalue: the largest cross product of two rows of A - x I at the bracket's middle
  decision      inlier iff n >= min_count, rank >= 2 and lambda0 <= flat * lambda1, on the brackets (None where they cannot tell)
  decisive      whether the exact quantities are further from their thresholds than a given error E (the tests pass the bound they
                ASSERT on the eigenvalues plus the zero rule's own threshold): rank <= 1 is always decisive (never an inlier); else
                lambda1 > 2 E — the threshold of eig1 > 0 is zero, so lambda1 itself is held against the error — and, for flat < 1,
                |lambda0 - flat lambda1| > (1 + flat) E
The catalogue: named lists of integer offset triples w, each replicated under axis permutations and the reflection w -> 65535 - w,
each variant in a cell of its own, as q = (cell + (w + 0.5) / 65536) * voxel — exact doubles at voxel = 0.5, for which
moment_offset returns w exactly."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np

VOXEL = 0.5
TOP = 65535
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
EPS = 2.0 ** -52


# ---- the ten words and the exact matrix ------------------------------------------------------------------------------------------------
def words(w):
    """the ten words of the points with offsets w (n, 3), as Python integers"""
    w = [[int(v) for v in p] for p in np.asarray(w).reshape(-1, 3).tolist()]
    out = [len(w)] + [sum(p[a] for p in w) for a in range(3)] + [sum(p[a] * p[b] for p in w) for a, b in PAIRS]
    assert all(0 <= v < 2 ** 64 for v in out)
    return out


def matrix(M):
    """A = n S2 - S1 S1^T = n^2 C, a 3 x 3 list of Python integers"""
    M = [int(v) for v in M]
    n, S1 = M[0], M[1:4]
    A = [[0] * 3 for _ in range(3)]
    for j, (a, b) in enumerate(PAIRS):
        A[a][b] = A[b][a] = n * M[4 + j] - S1[a] * S1[b]
    return A


def _minor(A, r, c):
    (r0, r1), (c0, c1) = [i for i in range(3) if i != r], [i for i in range(3) if i != c]
    return A[r0][c0] * A[r1][c1] - A[r0][c1] * A[r1][c0]


def invariants(A):
    """(trace, the sum of the principal 2 x 2 minors, the determinant): x^3 - t x^2 + m x - d is the characteristic polynomial"""
    t = A[0][0] + A[1][1] + A[2][2]
    m = _minor(A, 0, 0) + _minor(A, 1, 1) + _minor(A, 2, 2)
    d = A[0][0] * _minor(A, 0, 0) - A[0][1] * _minor(A, 0, 1) + A[0][2] * _minor(A, 0, 2)
    return t, m, d


def rank(A):
    if not any(v for row in A for v in row):
        return 0
    if not any(_minor(A, r, c) for r in range(3) for c in range(3)):
        return 1
    return 2 if invariants(A)[2] == 0 else 3


def _below(inv, j, D):
    """how many eigenvalues are < j / D, times counted as often as they occur: the sign changes of (1, t, m, d) of A - (j / D) I, each
    invariant scaled by the power of D that makes it an integer"""
    t, m, d = inv
    seq = [1, t * D - 3 * j, m * D * D - 2 * t * j * D + 3 * j * j, d * D ** 3 - m * j * D * D + t * j * j * D - j ** 3]
    signs = [v > 0 for v in seq if v != 0]
    return sum(1 for a, b in zip(signs, signs[1:]) if a != b)


def brackets(A, bits=96):
    """[(lo, hi)] x 3 as Fractions, ascending, in A's units: lo <= lambda_k <= hi, hi - lo <= 2^-bits of the trace (and at most 1)"""
    inv = invariants(A)
    t, rk = inv[0], rank(A)
    D = 1 << max(0, bits - max(t, 1).bit_length() + 1)
    out = []
    for k in range(3):
        if k < 3 - rk:
            out.append((Fraction(0), Fraction(0)))
            continue
        lo, hi = 0, (t + 1) * D  # (_below(lo) = 0 <= k: A is positive semi-definite; _below(hi) = 3 > k)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _below(inv, mid, D) > k:
                hi = mid
            else:
                lo = mid
        out.append((Fraction(lo, D), Fraction(hi, D)))
    return out


class Spectrum:
    """the exact side of one row: n, A, rank, the brackets in C's units (lo[k], hi[k]) and their middles as floats (lam)"""

    def __init__(self, M):
        self.M = [int(v) for v in M]
        self.n = self.M[0]
        self.A = matrix(self.M)
        self.rank = rank(self.A)
        self.in_A = brackets(self.A)
        n2 = self.n * self.n
        self.lo = [b[0] / n2 for b in self.in_A]
        self.hi = [b[1] / n2 for b in self.in_A]
        self.lam = [float((a + b) / 2) for a, b in zip(self.lo, self.hi)]
        self.floor = EPS * max(self.M[4], self.M[7], self.M[9]) / self.n  # 2^-52 max(S2_aa / n): the unit of the cancellation floor

    def vector(self, k):
        """a unit eigenvector (fp64) of eigenvalue k, meaningful where that eigenvalue is simple"""
        x = (self.in_A[k][0] + self.in_A[k][1]) / 2
        B = [[Fraction(self.A[r][c]) - (x if r == c else 0) for c in range(3)] for r in range(3)]
        best, best_n = None, -1
        for r0, r1 in ((0, 1), (0, 2), (1, 2)):
            a, b = B[r0], B[r1]
            v = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            nn = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
            if nn > best_n:
                best, best_n = v, nn
        big = max(abs(c) for c in best)
        v = np.array([float(c / big) for c in best])
        return v / np.linalg.norm(v)

    def certificate(self, eig, v, voxel=VOXEL):
        """(||r|| / ||v|| in C's units as a float, ||v||^2 as a Fraction, lambda' in C's units as a Fraction) of the claimed pair:
        eig in m^2 and v three numbers, all taken as the exact binary rationals they are"""
        s = Fraction(voxel) / 65536
        lam = Fraction(float(eig)) / (s * s)
        v = [Fraction(float(c)) for c in v]
        n2 = self.n * self.n
        r = [sum(Fraction(self.A[a][b], n2) * v[b] for b in range(3)) - lam * v[a] for a in range(3)]
        vv = sum(c * c for c in v)
        return math.sqrt(sum(c * c for c in r) / vv), vv, lam

    def gap(self, own, lam):
        """the distance of lam (a Fraction, C's units) to the exact eigenvalues NOT in `own` (indices), a lower bound from the
        brackets: Davis-Kahan's denominator for the angle to the span of the eigenvectors in `own`"""
        return float(min(max(self.lo[j] - lam, lam - self.hi[j], Fraction(0)) for j in range(3) if j not in own))

    def inlier(self, min_count, flat):
        """the exact decision; None where the brackets cannot tell (they are 2^-96 of the trace wide)"""
        if self.n < min_count or self.rank < 2:
            return False
        if flat >= 1:
            return True  # (lambda0 <= lambda1 always)
        f = Fraction(float(flat))
        if self.hi[0] <= f * self.lo[1]:
            return True
        if self.lo[0] > f * self.hi[1]:
            return False
        return None

    def error(self, a, c):
        """a lambda2 + c floor, in C's units: the form of every bound on an eigenvalue"""
        return a * self.lam[2] + c * self.floor

    def decisive(self, flat, E):
        """whether the exact quantities are further from the gate's thresholds than E (C's units)"""
        if self.rank <= 1:
            return True
        if not float(self.lo[1]) > 2 * E:
            return False
        if flat >= 1:
            return True
        return abs(self.lam[0] - flat * self.lam[1]) > (1 + flat) * E

    def margin(self, flat):
        """(lambda1 / lambda2, |lambda0 - flat lambda1| / lambda2): what `decisive` compares with the error, as shares of lambda2"""
        l2 = self.lam[2] if self.lam[2] > 0 else 1.0
        return self.lam[1] / l2, abs(self.lam[0] - flat * self.lam[1]) / l2


# ---- eig3_sym's branches, restated on the exact spectrum ------------------------------------------------------------------------------
def branches(sp, margin=1.01):
    """the set of branch names of csrc/common/eig3.h's eig3_sym this row reaches WITH MARGIN (a choice between two quantities counts
    only where one exceeds the other by 1 %), from the exact spectrum and fp64 arithmetic on it — not bit-faithful, nor meant to be.
    "double" in particular is restated as an EXACT double root, while the solver takes that branch on `d0 <= 2 eps d1` of its computed
    roots, which near a double root carry sqrt(eps) unless q clamps to zero (it does for the lines along an axis): the census shows
    that candidates are there, not that the branch runs.  The witness that it runs is a mutant: with the re-normalisation of that
    branch taken out of a scratch copy of eig3.h, the unit-length assertion of tests/test_host_map_surfels_exact.py failed
    (| ||n||^2 - 1 | = 5.0)."""
    out = set()
    l = sp.lam
    if sp.rank == 0 or (sp.lo[0] == sp.lo[2] and sp.hi[0] == sp.hi[2] and float(sp.hi[2] - sp.lo[0]) <= 1e-20 * max(l[2], 1e-300)):
        return {"identity"}
    if l[2] - l[0] <= 1e-12 * l[2]:
        return {"identity"}  # (an exact triple root)
    d0, d1 = l[2] - l[1], l[1] - l[0]
    if d0 > margin * d1:
        k, lo = 2, 0
        out.add("k=2")
    elif d1 > margin * d0:
        k, lo = 0, 2
        out.add("k=0")
    else:
        return out
    double = min(d0, d1) <= 1e-20 * l[2]
    if double:
        out.add("double")
    n2 = float(sp.n) ** 2
    for which in ((k,) if double else (k, lo)):
        B = np.array([[sp.A[r][c] / n2 - (l[which] if r == c else 0.0) for c in range(3)] for r in range(3)])
        dg = np.abs(np.diag(B))
        i0 = int(np.argmax(dg))
        if dg[i0] < margin * np.sort(dg)[1]:
            continue
        out.add("i0=%d" % i0)
        repr_, c1, c2 = B[:, i0], B[:, (i0 + 1) % 3], B[:, (i0 + 2) % 3]
        n1, n2_ = float(np.sum(np.cross(repr_, c1) ** 2)), float(np.sum(np.cross(repr_, c2) ** 2))
        if n1 > margin * n2_:
            out.add("cross=1")
        elif n2_ > margin * n1:
            out.add("cross=2")
    return out


ALL_BRANCHES = {"identity", "k=0", "k=2", "double", "i0=0", "i0=1", "i0=2", "cross=1", "cross=2"}


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------
def _line(direction, n, step):
    return np.outer(np.arange(n) * step, np.asarray(direction)).astype(np.int64)


def _grid(m):
    return np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int64)


def _noisy_plane(rng, ratio, n=400, extent=60000):
    xy = rng.integers(0, extent, size=(n, 2))
    z = np.rint(0.07 * xy[:, 0] + 0.05 * xy[:, 1] + rng.normal(0.0, ratio * extent, n)).astype(np.int64)
    return np.column_stack([xy, z - z.min()])


def _shapes():
    """name -> offsets (n, 3) int64, smallest coordinate 0 on every axis: shapes that `_placed` moves about the voxel"""
    rng = np.random.default_rng(2024)
    g = _grid(10)
    s = {}
    s["identical3"] = np.zeros((3, 3), np.int64)
    for n in (3, 100):
        step = 9000 if n == 3 else 190
        s["line_axis%d" % n] = _line((1, 0, 0), n, step)
        s["line_face%d" % n] = _line((1, 1, 0), n, step)
        s["line_531_%d" % n] = _line((5, 3, 1), n, step // 5)
    j = _line((5, 3, 1), 100, 38) + rng.integers(-1, 2, size=(100, 3))
    s["line_531_jitter"] = j - j.min(axis=0)
    s["plane_axis"] = np.column_stack([100 * g[:, 0], 130 * g[:, 1], np.zeros(100, np.int64)])
    s["plane_tilted"] = np.column_stack([100 * g[:, 0], 130 * g[:, 1], 100 * g[:, 0] + 130 * g[:, 1]])
    s["plane_floored"] = np.column_stack([37 * g[:, 0], 53 * g[:, 1], (37 * g[:, 0] + 53 * g[:, 1]) // 2])
    s["square"] = np.array([[0, 0, 0], [20000, 0, 0], [0, 20000, 0], [20000, 20000, 0]], np.int64)
    s["cube"] = np.array(list(itertools.product((0, 20000), repeat=3)), np.int64)
    for k, ratio in enumerate((1e-2, 1e-4, 1e-6)):
        s["noisy_plane_1e-%d" % (2 * k + 2)] = _noisy_plane(rng, ratio)
    s["one"] = np.array([[0, 0, 0]], np.int64)
    s["two"] = np.array([[0, 0, 0], [300, 200, 100]], np.int64)
    s["triangle"] = np.array([[0, 700, 0], [900, 0, 200], [300, 400, 1100]], np.int64)
    s["tetra"] = np.array([[0, 700, 0], [900, 0, 200], [300, 400, 1100], [1000, 1000, 50]], np.int64)
    return s


def _placed(d, where):
    room = TOP - d.max(axis=0)
    return d + {"bottom": 0 * room, "middle": room // 2, "top": room}[where]


PERMUTATIONS = list(itertools.permutations(range(3)))


def _variants(w, full=True):
    """w under the six axis permutations and the reflection w -> 65535 - w (full), or as it is and reflected"""
    out = []
    for p in (PERMUTATIONS if full else PERMUTATIONS[:1]):
        for mirror in (False, True):
            v = w[:, list(p)]
            out.append(("%s%s" % ("".join("xyz"[a] for a in p), "-" if mirror else "+"), TOP - v if mirror else v))
    return out


def _cell_key(cell):
    return sum((int(cell[a]) + (1 << 20)) << (21 * a) for a in range(3))


class Entry:
    def __init__(self, name, w, cell):
        self.name, self.w, self.cell = name, np.ascontiguousarray(w, np.int64), tuple(int(c) for c in cell)
        assert self.w.min() >= 0 and self.w.max() <= TOP, name
        self.n = self.w.shape[0]
        self.key = _cell_key(self.cell)
        self.M = words(self.w)

    @functools.cached_property
    def spectrum(self):
        return Spectrum(self.M)

    def points(self, voxel=VOXEL):
        return (np.array(self.cell, np.float64) + (self.w.astype(np.float64) + 0.5) / 65536.0) * voxel

    def probe(self, voxel=VOXEL):
        """the fp64 centroid of the row, a point of its own cell"""
        m = np.array([self.M[1 + a] / self.n for a in range(3)])
        return (np.array(self.cell, np.float64) + (m + 0.5) / 65536.0) * voxel


@functools.lru_cache(maxsize=None)
def catalogue():
    """the list of Entry, in the order their points are folded.  Populations of more than 1 000 points are not replicated under all
    twelve variants (the whole catalogue stays under 300 000 points, and 12 x 3 x 4 096 alone is half of that): 4 096 uniform points
    come as they are and reflected in the middle and at the top and as they are at the bottom, 4 096 identical points once per
    place, the two populations of 100 000 once."""
    rng = np.random.default_rng(7)
    named = []
    for name, d in _shapes().items():
        for where in ("middle", "top", "bottom"):
            for tag, w in _variants(_placed(d, where)):
                named.append(("%s/%s/%s" % (name, where, tag), w))
    corners = np.array([[0, 0, 0]] * 3 + [[TOP, TOP, TOP]], np.int64)
    named += [("three_and_one/" + tag, w) for tag, w in _variants(corners)]
    ball = rng.integers(0, 20000, size=(4096, 3))
    for where in ("middle", "top"):
        named += [("uniform4096/%s/%s" % (where, tag), w) for tag, w in _variants(_placed(ball, where), full=False)]
        named.append(("identical4096/%s" % where, _placed(np.zeros((4096, 3), np.int64), where) - np.array([11, 7, 3]) * (where == "top")))
    named.append(("top_cube_100000", rng.integers(TOP - 2, TOP + 1, size=(100000, 3))))
    thin = np.column_stack([rng.integers(63000, TOP + 1, size=(100000, 2)), rng.integers(TOP - 1, TOP + 1, size=100000)])
    named.append(("top_thin_plane_100000", thin))
    named.append(("uniform4096/bottom/xyz+", _placed(ball, "bottom")))
    # a cell of its own for each, two apart; the first three at both ends of the key range and at a negative cell
    special = [(-(1 << 20),) * 3, ((1 << 20) - 1,) * 3, (-1, -1, -1)]
    out = []
    for i, (name, w) in enumerate(named):
        cell = special[i] if i < 3 else (2 * (i % 400) - 300, 2 * (i // 400) + 4, -7)
        out.append(Entry(name, w, cell))
    assert len({e.key for e in out}) == len(out)
    return out


def cloud(entries=None, voxel=VOXEL):
    """every point of the catalogue, (N, 3) fp64, to fold under the identity"""
    return np.concatenate([e.points(voxel) for e in (entries or catalogue())])


def by_row(keys, entries=None):
    """the entries in the order of a map's rows, from its downloaded stored keys"""
    of = {e.key: e for e in (entries or catalogue())}
    return [of[int(k)] for k in np.asarray(keys).tolist()]


# ---- the checks both sides share --------------------------------------------------------------------------------------------------------
def eig_errors(entries, eig, voxel=VOXEL):
    """(err (M, 3), lambda2 (M,), floor (M,)), all in C's units: the distance of every delivered eigenvalue (m^2, float32, taken as
    the exact rational it is) from the bracket of the exact one, and the two quantities a bound on it is made of"""
    s2 = (voxel / 65536.0) ** 2
    err = np.empty((len(entries), 3))
    l2, fl = np.empty(len(entries)), np.empty(len(entries))
    for r, e in enumerate(entries):
        sp = e.spectrum
        for k in range(3):
            x = Fraction(float(eig[r, k])) / Fraction(s2)
            err[r, k] = float(max(x - sp.hi[k], sp.lo[k] - x, Fraction(0)))
        l2[r], fl[r] = sp.lam[2], sp.floor
    return err, l2, fl
