"""A plain restatement of motion compensation from per-point timestamps (madicp_cloud_deskew_stamped, its host twin
madicp_host_deskew_stamped) and the inputs that try it.

TEST INFRASTRUCTURE ONLY.  The time model is the reference's own (pipeline.cpp:99-117): CHUNKS = 1024 chunk times, t_0 = -1/hz,
then repeated addition of (1/hz) / 1023; one pose [expMapSO3(omega t_k), v t_k] per chunk, with the first-order branch below
theta^2 < 1e-8 (lie_algebra.h:39-52).  What is new is where a point's chunk comes from — its own stamp s in [0, 1]:

    s is NaN                     -> 1023   (time unknown: taken as the scan's end, the frame the pose refers to)
    q = floor(s * 1023.0 + 0.5)  -> 0 if q <= 0, 1023 if q >= 1023, else int(q)        (fp64, no fused multiply-add)

and out[i] = pose[k_i] * p[i] in INPUT order, each row as  P[9 + r] + (P[3r] x + (P[3r+1] y + P[3r+2] z)).

  times(hz)                 the running chunk time (math, repeated addition)
  chunk_poses(vel, hz)      (1024, 12): R row-major | t, libm through `math`
  first_order_chunks(...)   which chunks take the first-order branch
  chunk_of(s)               the rule above, elementwise
  compensate(pts, s, ...)   the compensated cloud
  stamp families, the four velocities, poses_for(vel, hz), physical_scan(...)
"""
import math

import numpy as np

CHUNKS = 1024                      # tools/constants.h


def times(sensor_hz, count=CHUNKS):
    ts = 1. / sensor_hz
    delta = ts / float(CHUNKS - 1)
    out = np.empty(count)
    t = -ts
    for k in range(count):
        out[k] = t
        t += delta
    return out


def exp_so3(w):
    """lie_algebra.h:39-52.  Returns (R (3,3), first_order)."""
    w0, w1, w2 = (float(x) for x in w)
    th2 = (w0 * w0 + w1 * w1) + w2 * w2
    W = np.array([[0.0, -w2, w1], [w2, 0.0, -w0], [-w1, w0, 0.0]])
    if th2 < 1e-8:
        return np.eye(3) + W, True
    th = math.sqrt(th2)
    K = W / th
    omc = 2.0 * math.sin(th / 2.0) * math.sin(th / 2.0)
    return (np.eye(3) + math.sin(th) * K) + (omc * K) @ K, False


def chunk_poses(vel, sensor_hz):
    vel = np.asarray(vel, dtype=np.float64)
    P = np.empty((CHUNKS, 12))
    for k, t in enumerate(times(sensor_hz)):
        dx = vel * t
        R, _ = exp_so3(dx[3:])
        P[k, :9] = R.reshape(-1)
        P[k, 9:] = dx[:3]
    return P


def first_order_chunks(vel, sensor_hz):
    vel = np.asarray(vel, dtype=np.float64)
    return np.array([exp_so3(vel[3:] * t)[1] for t in times(sensor_hz)])


def chunk_of(s):
    s = np.atleast_1d(np.asarray(s, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(s * 1023.0 + 0.5)
    k = np.empty(s.shape, dtype=np.int64)
    nan = s != s
    lo = ~nan & (q <= 0.0)
    hi = ~nan & (q >= 1023.0)
    mid = ~(nan | lo | hi)
    k[nan] = 1023
    k[lo] = 0
    k[hi] = 1023
    k[mid] = q[mid].astype(np.int64)
    return k


def compensate(pts, stamps, vel, sensor_hz):
    pts = np.asarray(pts, dtype=np.float64)
    P = chunk_poses(vel, sensor_hz)[chunk_of(stamps)]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty_like(pts)
    for r in range(3):
        out[:, r] = P[:, 9 + r] + (P[:, 3 * r] * x + (P[:, 3 * r + 1] * y + P[:, 3 * r + 2] * z))
    return out


# ---- stamps --------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, 1.0, math.nextafter(1.0, 0.0), -1.0, 2.0, math.nan, math.inf, -math.inf])
SPECIAL_CHUNKS = np.array([0, 0, 1023, 1023, 0, 1023, 1023, 1023, 0])


def centres():
    return np.arange(CHUNKS, dtype=np.float64) / 1023.0


def boundaries():
    """(1023, 3): the boundary (k + 0.5) / 1023 between chunks k and k + 1, its lower and its upper neighbour."""
    b = (np.arange(CHUNKS - 1, dtype=np.float64) + 0.5) / 1023.0
    return np.stack([np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)], axis=1)


def family(name, n=None, seed=0):
    """Stamps of one family; `n` given: cut or cyclically repeated to n values.  Always shuffled: the input order of a cloud
    is not its time order."""
    rng = np.random.default_rng([seed, ["uniform", "centres", "boundaries", "specials"].index(name)])
    if name == "uniform":
        s = rng.uniform(0.0, 1.0, n if n is not None else 4096)
    elif name == "centres":
        s = centres()
    elif name == "boundaries":
        s = boundaries().reshape(-1)
    else:
        s = SPECIALS.copy()
    s = s[rng.permutation(s.size)]
    if n is not None and s.size != n:
        s = np.resize(s, n)
    return np.ascontiguousarray(s)


def mixed_stamps(n, seed=0):
    """n stamps drawn from all four families at once, in shuffled order: a random draw from {specials, boundaries with their
    neighbours, centres, 1024 uniform values}, topped up with uniform values when n is larger than that pool."""
    rng = np.random.default_rng([seed, n])
    pool = np.concatenate([SPECIALS, boundaries().reshape(-1), centres(), rng.uniform(0.0, 1.0, 1024)])
    pool = pool[rng.permutation(pool.size)]
    s = pool[:n] if n <= pool.size else np.concatenate([pool, rng.uniform(0.0, 1.0, n - pool.size)])
    return np.ascontiguousarray(s[rng.permutation(n)])


# ---- velocities ----------------------------------------------------------------------------------------------------------------
V_LIN = np.array([20.0, 1.0, -0.5])
W_DIR = np.array([0.05, -0.1, 0.6]) / np.linalg.norm([0.05, -0.1, 0.6])
VELOCITIES = {
    "zero": np.zeros(6),
    "first_order": np.concatenate([V_LIN, 5e-4 * W_DIR]),   # theta^2 <= (5e-4 * 0.1)^2 = 2.5e-9 < 1e-8 over the whole table
    "rodrigues": np.concatenate([V_LIN, 0.6 * W_DIR]),      # Rodrigues everywhere but the last two chunks, where t -> 0
    "crossing": np.concatenate([V_LIN, 0.01 * W_DIR]),      # theta^2 = 1e-8 at |t| = 0.01 s: chunk 921 of 1024 at 10 Hz
}
PHYSICAL_VEL = np.array([20.0, 1.0, -0.5, 0.05, -0.1, 0.6])  # the sign-convention test's motion
HZ = 10.0


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + math.sin(th) / th * W + (1.0 - math.cos(th)) / (th * th) * (W @ W)


def poses_for(vel, sensor_hz):
    """(T_prev, T_now) as 4x4 whose naive velocity (pipeline.cpp:82-86) is `vel` up to the log map's rounding."""
    vel = np.asarray(vel, dtype=np.float64)
    T = np.eye(4)
    T[:3, :3] = rodrigues(vel[3:] / sensor_hz)
    T[:3, 3] = vel[:3] / sensor_hz
    return np.eye(4), T


def physical_scan(n, vel, sensor_hz, r_max=60.0, seed=5):
    """World points w (in the scan-end frame) seen by a sensor that moves with the naive model: the point acquired at
    tau_i = -(1 - s_i) / hz is measured as  p_i = R(omega tau_i)^T (w_i - v tau_i).  Returns (p, s, w, bound): compensating p
    with the true velocity must give w back within half a chunk of motion,
    bound = 1.1 * (|v| + |omega| r_max) * (1 / hz) / 1023 / 2  (the 10 % is for the second-order term)."""
    vel = np.asarray(vel, dtype=np.float64)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    w = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(4.0, r_max, (n, 1))
    s = rng.uniform(0.0, 1.0, n)
    tau = -(1.0 - s) / sensor_hz
    p = np.empty_like(w)
    for i in range(n):
        p[i] = rodrigues(vel[3:] * tau[i]).T @ (w[i] - vel[:3] * tau[i])
    bound = 1.1 * (np.linalg.norm(vel[:3]) + np.linalg.norm(vel[3:]) * r_max) * (1.0 / sensor_hz) / 1023.0 / 2.0
    return np.ascontiguousarray(p), s, w, bound
