"""The registration of a scan against the voxel map's surfels (include/madicp_hip.h: madicp_map_register_cloud; the rule is
mad_icp_amd/csrc/common/map_align.h) restated in numpy, and the scene the host and the device tests share.  Everything in float64
or integers, elementwise (numpy does not fuse).  The surfel columns — centroid, normal, eig (m, 3) float32, count (m,) uint32 — are
an INPUT: the side under test hands over its own, so the last bits of its eigen-solve are no part of the comparison.
  row, d2    map_query_ref.query: the same rule as the query, not a second one
  inlier     row >= 0, d2 <= max_dist^2, count >= min_count, eig1 > 0, eig0 <= flat * eig1
             (eig1 > 0 stands on map_surfel's ZERO RULE, restated as `zero_at`: an eigenvalue w of the covariance, in offset units
             squared, is delivered as +0.0 unless w > 2^-24 w2 + 4 * 2^-52 max(S2_aa / n) — so a line or a point has eig1 == 0)
  e, J       e = n0 (q0 - c0) + (n1 (q1 - c1) + n2 (q2 - c2)); m = n^T R; J = [m, p x m]
  terms      s = |e| > rho ? rho / |e| : 1; H(r, c) = (s J[r]) J[c], r >= c, packed column by column | b[r] = (s J[r]) e | (s e) e
  the sum    `tree`: pad with +0.0 to the next power of two, then x = x[0::2] + x[1::2] until one vector is left — by reshapes
  the step   numpy.linalg.solve and Rodrigues with the reference's first-order branch (lie_algebra.h:39-52), X <- X * dX
`jacobian_fd` holds J to central finite differences of `errors` under X * exp(dx): the sign and the side of the perturbation."""
import functools

import numpy as np

import cloud_export_ref as E
import map_query_ref as Q

VOXEL = 0.5
TERMS = 28
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4097, 65793]  # wavefront, workgroup, second and third tree level: 65 793 = 257 rows + 1
DEFAULT = dict(reach=1, max_dist=np.inf, rho=np.inf, min_count=3, flat=1.0)            # the neutral parameters
GATED = dict(reach=1, max_dist=0.45, rho=0.03, min_count=40, flat=0.3)                 # every gate and the kernel at work
SEED = 23  # the committed seed: along the five GATED rounds at n = 4 097 gate_margins stays above 1e-3 (3.9e-3 for d2, 0.42 for the
#            eigenvalues; of the seeds 20 .. 39 tried, 20 and 22 did not) — tests/test_host_map_align.py asserts it


ZERO_SHARE, ZERO_FLOOR = 2.0 ** -24, 4.0  # voxel_moments.h: kSurfelZeroShare, kSurfelZeroFloor


def zero_at(mom, w2):
    """the zero rule's threshold per row, in offset units squared: mom (M, 10) the ten words, w2 (M,) the largest eigenvalue"""
    m = np.asarray(mom).astype(np.float64)
    return ZERO_SHARE * np.asarray(w2, np.float64) + ZERO_FLOOR * 2.0 ** -52 * (m[:, [4, 7, 9]] / m[:, 0:1]).max(axis=1)


def tree(x):
    """(n, TERMS) -> (TERMS,): the adjacent-pair binary tree in row order over the rows padded with +0.0 to a power of two"""
    x = np.ascontiguousarray(x, np.float64).reshape(-1, TERMS)
    n = x.shape[0]
    if n == 0:
        return np.zeros(TERMS)
    size = 1
    while size < n:
        size *= 2
    pad = np.zeros((size, TERMS))
    pad[:n] = x
    x = pad
    while x.shape[0] > 1:
        x = x.reshape(-1, 2, TERMS)
        x = x[:, 0, :] + x[:, 1, :]
    return x[0]


def unpack(total):
    """the 28 sums -> (H (6, 6) symmetric, b (6,), chi2)"""
    H = np.zeros((6, 6))
    v = 0
    for c in range(6):
        for r in range(c, 6):
            H[r, c] = H[c, r] = total[v]
            v += 1
    return H, np.array(total[21:27]), float(total[27])


def _jacobian(p, R, nr):
    m = [nr[:, 0] * R[0, k] + (nr[:, 1] * R[1, k] + nr[:, 2] * R[2, k]) for k in range(3)]
    return m + [p[:, 1] * m[2] - p[:, 2] * m[1], p[:, 2] * m[0] - p[:, 0] * m[2], p[:, 0] * m[1] - p[:, 1] * m[0]]


def errors(surfels, row, cloud, R, t):
    """e of every point against the surfel of ITS GIVEN row (row >= 0), whatever the gates say"""
    centroid, normal = surfels[0], surfels[1]
    q = E.positions(cloud, R, t)
    c, nr = centroid[row].astype(np.float64), normal[row].astype(np.float64)
    return nr[:, 0] * (q[:, 0] - c[:, 0]) + (nr[:, 1] * (q[:, 1] - c[:, 1]) + nr[:, 2] * (q[:, 2] - c[:, 2]))


def linearize(rows, keys, surfels, cloud, R, t, voxel=VOXEL, reach=1, max_dist=np.inf, rho=np.inf, min_count=3, flat=1.0):
    """-> dict(counts (4,), row (n,) int32, e (n,), total (28,), H, b, chi2, inlier (n,) bool, d2 (n,))"""
    centroid, normal, eig, count = surfels
    p = np.ascontiguousarray(cloud, np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    n, m = p.shape[0], np.asarray(keys).reshape(-1).shape[0]
    ans = Q.query(rows, keys, p, R, t, voxel, reach, max_dist)
    row, d2 = ans["row"], ans["d2"]
    terms, e = np.zeros((n, TERMS)), np.zeros(n)
    inlier = np.zeros(n, bool)
    if n and m:
        j = np.where(row >= 0, row, 0)
        md2 = np.float64(max_dist) * np.float64(max_dist)
        e0, e1 = eig[j, 0].astype(np.float64), eig[j, 1].astype(np.float64)
        with np.errstate(all="ignore"):
            inlier = (row >= 0) & (d2 <= md2) & (count[j] >= min_count) & (e1 > 0.0) & (e0 <= np.float64(flat) * e1)
            ee = errors(surfels, j, p, R, t)
            J = _jacobian(p, R, normal[j].astype(np.float64))
            a = np.abs(ee)
            s = np.where(a > rho, np.float64(rho) / a, 1.0)
            sJ = [s * Jr for Jr in J]
            v = 0
            for c in range(6):
                for r in range(c, 6):
                    terms[:, v] = sJ[r] * J[c]
                    v += 1
            for r in range(6):
                terms[:, 21 + r] = sJ[r] * ee
            terms[:, 27] = (s * ee) * ee
        terms[~inlier] = 0.0
        e = np.where(inlier, ee, 0.0)
    total = tree(terms)
    H, b, chi2 = unpack(total)
    counts = np.array(list(ans["counts"]) + [int(np.count_nonzero(inlier))], np.uint64)
    return dict(counts=counts, row=row, e=e, total=total, H=H, b=b, chi2=chi2, inlier=inlier, d2=d2)


def exp_so3(w):
    """lie_algebra.h:39-52: I + skew(w) below |w|^2 < 1e-8, Rodrigues from there on"""
    w = np.asarray(w, np.float64)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    th2 = float(w @ w)
    if th2 < 1e-8:
        return np.eye(3) + W
    th = np.sqrt(th2)
    K = W / th
    return np.eye(3) + np.sin(th) * K + (2.0 * np.sin(th / 2.0) ** 2) * (K @ K)


def rodrigues(w):
    """the true exponential (for poses and finite differences)"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + W
    K = W / th
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def step(H, b, R, t):
    """one update: dx = H^-1 (-b) (0 for an all-zero H), X <- X * (exp(dx[3:]), dx[:3]) -> (R, t)"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    dx = np.linalg.solve(H, -b) if np.any(H) else np.zeros(6)
    return R @ exp_so3(dx[3:]), R @ dx[:3] + t


def register(rows, keys, surfels, cloud, R, t, iterations, voxel=VOXEL, **params):
    """-> (R, t, [linearize() at X_0 .. X_iterations], [(R, t) of X_0 .. X_iterations])"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    lins, poses = [], []
    for k in range(iterations + 1):
        lin = linearize(rows, keys, surfels, cloud, R, t, voxel, **params)
        lins.append(lin)
        poses.append((R, t))
        if k < iterations:
            R, t = step(lin["H"], lin["b"], R, t)
    return R, t, lins, poses


def jacobian_fd(surfels, row, cloud, R, t, h=1e-6):
    """-> (J analytic (n, 6), J by central differences of `errors` under X * exp(dx) (n, 6)) for points with the given rows"""
    p = np.ascontiguousarray(cloud, np.float64).reshape(-1, 3)
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    J = np.stack(_jacobian(p, R, surfels[1][row].astype(np.float64)), axis=1)
    fd = np.zeros_like(J)
    for k in range(6):
        e = []
        for sgn in (1.0, -1.0):
            dx = np.zeros(6)
            dx[k] = sgn * h
            e.append(errors(surfels, row, p, R @ rodrigues(dx[3:]), R @ dx[:3] + t))
        fd[:, k] = (e[0] - e[1]) / (2.0 * h)
    return J, fd


def gate_margins(lin, surfels, max_dist, flat):
    """the smallest relative distance of a gate quantity from its threshold over the matched points of a linearisation: (d2 against
    max_dist^2, eig0 against flat * eig1) — inf where the gate has nothing to decide"""
    row = lin["row"]
    hit = row >= 0
    out = [np.inf, np.inf]
    if np.any(hit):
        md2 = float(max_dist) ** 2
        if np.isfinite(md2) and md2 > 0:
            out[0] = float(np.min(np.abs(lin["d2"][hit] - md2) / md2))
        eig = surfels[2][np.unique(row[hit])].astype(np.float64)
        thr = flat * eig[:, 1]
        ok = thr > 0
        if np.any(ok):
            out[1] = float(np.min(np.abs(eig[ok, 0] - thr[ok]) / thr[ok]))
    return tuple(out)


def pose_distance(Ra, ta, Rb, tb):
    """(metres, radians) between two poses"""
    Ra, Rb = np.asarray(Ra).reshape(3, 3), np.asarray(Rb).reshape(3, 3)
    d = Ra.T @ Rb
    return float(np.linalg.norm(np.asarray(ta) - np.asarray(tb))), float(np.arccos(np.clip((np.trace(d) - 1.0) / 2.0, -1.0, 1.0)))


# ---- the scene: a room corner — three mutually orthogonal noisy planes --------------------------------------------------------------
CORNER = np.array([0.23, 0.31, 0.17])  # (off the voxel faces)
SIDE, NOISE = 6.0, 0.02
FOLDS, FOLD_POINTS = 4, 9000
TRUE_POSE = (rodrigues([0.3, -0.2, 0.5]), np.array([1.0, -2.0, 0.5]))
OFFSET = (rodrigues([0.010, -0.012, 0.015]), np.array([0.03, -0.02, 0.04]))  # about a degree and a few centimetres


def corner_points(n, seed, margin=0.0):
    """n world-frame points, point i on plane i % 3 (so every prefix sees all three), Gaussian noise along the plane's normal"""
    rng = np.random.default_rng(seed)
    p = CORNER + rng.uniform(margin, SIDE - margin, size=(n, 3))
    axis = np.arange(n) % 3
    p[np.arange(n), axis] = CORNER[axis] + rng.normal(size=n) * NOISE
    return p


def map_folds():
    """the clouds folded into the map, under the identity"""
    return [corner_points(FOLD_POINTS, SEED + 1 + k) for k in range(FOLDS)]


@functools.lru_cache(maxsize=None)
def scan(n, seed=SEED):
    """a fresh sample of the planes in the SENSOR frame of TRUE_POSE (half a metre inside the map's extent)"""
    return Q.into_cloud_frame(corner_points(n, seed + 100 + n, margin=0.5), *TRUE_POSE)


def start_pose():
    """TRUE_POSE * OFFSET: where a registration starts"""
    R, t = TRUE_POSE
    return R @ OFFSET[0], R @ OFFSET[1] + t
