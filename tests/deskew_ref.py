"""A plain restatement of the chunk assignment of Pipeline::deskew (pipeline.cpp:89-119) and the clouds that make it work.

TEST INFRASTRUCTURE ONLY.  The reference sorts the points by azimuth and walks them from the largest azimuth down; it moves on
to the next time chunk AT MOST ONCE per point, when the point's azimuth is below the running threshold.  After an azimuth gap
wider than one threshold (2 pi / 1024) the walk therefore LAGS: it is behind the chunk the point's azimuth belongs to for as
many points as it skipped thresholds.  The device computes the same chunks as a prefix minimum
(mad_icp_amd/csrc/hip/frontend.hip.h: k_d = d + min(1, min_{j<=d}(T_j - j))), which only differs from the element itself while
the walk lags — so the clouds here are made to lag, and `walk()` says where they do.

  azimuths(pts)      math.atan2 per point (libm, what std::atan2 is; numpy.arctan2 may take a vectorised route)
  thresholds(count)  the reference's running `angle`: M_PI - resolution, then repeated subtraction
  times(hz, count)   the reference's running `t`: -1/hz, then repeated addition of (1/hz) / 1023
  walk(pts)          the literal loop: chunk k_d and T_d per walk position d (0 = largest azimuth), and a census
  cloud_from_azimuths / the *_azimuths makers: clouds whose math.atan2 values are pairwise distinct and never +-0.0, so that
                     std::sort's order is the only possible one

tests/test_deskew_ref.py holds walk() to the oracle's and the host's deskew on every cloud family of
tests/test_gpu_frontend_edges.py; that file holds the device to both.
"""
import math

import numpy as np

CHUNKS = 1024                      # tools/constants.h
RESOLUTION = 2 * math.pi / float(CHUNKS)
TABLE = 1100                       # thresholds tabulated: past ~1024 they are below -pi and no azimuth undercuts them
WAVE, TILE, STRIP = 64, 1024, 262144  # the three carries of the device's prefix minimum (wavefront, workgroup tile, pmin_top strip)


def azimuths(pts):
    pts = np.asarray(pts, dtype=np.float64)
    return np.array([math.atan2(float(p[1]), float(p[0])) for p in pts], dtype=np.float64)


def thresholds(count=TABLE, first=None, resolution=RESOLUTION):
    """thr[k] = the running `angle` the (k+1)-th chunk change is decided against (pipeline.cpp:107,111)."""
    out = np.empty(count)
    angle = math.pi - resolution if first is None else first
    for k in range(count):
        out[k] = angle
        angle -= resolution
    return out


def times(sensor_hz, count=TABLE):
    """t[k] = the running time of chunk k (pipeline.cpp:103-104,112)."""
    ts = 1. / sensor_hz
    delta = ts / float(CHUNKS - 1)
    out = np.empty(count)
    t = -ts
    for k in range(count):
        out[k] = t
        t += delta
    return out


def walk(pts, strict=True, first=None):
    """The reference's walk over `pts` (n, 3).  Returns a dict:
      order   (n,) input row of every OUTPUT row (ascending azimuth: the reference writes its result in that order)
      az      (n,) azimuth by walk position d (descending)
      chunks  (n,) k_d: the chunk walk position d is compensated with
      T       (n,) T_d: thresholds above the azimuth of walk position d — where a walk that never lagged would be
      lag     (n,) k_d < T_d: the walk is behind the chunk of the point's azimuth;  lagging: how many positions are
      rises   number of d with T_d - d > T_{d-1} - (d-1): the prefix minimum differs from its element only after one
      lag_across / live_across
              {64: [...], 1024: [...], 262144: [...]}: the multiples b of each carry width with b-1 and b both lagging, and
              those where the result at b DEPENDS on what came before b:  min_{j<b}(T_j - j) < min(1, T_b - b)
    `strict` and `first` exist for the sensitivity check of tests/test_deskew_ref.py only (`<` -> `<=`, another start)."""
    az_in = azimuths(pts)
    n = az_in.size
    order = np.argsort(az_in, kind="stable")
    az_sorted = az_in[order]
    thr = thresholds(first=first)
    chunks = np.empty(n, dtype=np.int64)
    angle = math.pi - RESOLUTION if first is None else first
    k = 0
    for i in range(n - 1, -1, -1):                      # pipeline.cpp:108-119, literally
        a = az_sorted[i]
        if (a < angle) if strict else (a <= angle):
            angle -= RESOLUTION
            k += 1
        chunks[n - 1 - i] = k
    az_walk = az_sorted[::-1].copy()
    # thresholds strictly decrease: T = #{k : a < thr[k]}
    T = np.searchsorted(-thr, -az_walk, side="left").astype(np.int64)
    d = np.arange(n, dtype=np.int64)
    g = T - d
    lag = chunks < T
    rises = int((np.diff(g) > 0).sum())
    pmin = np.minimum.accumulate(g) if n else g
    lag_across, live_across = {}, {}
    for width in (WAVE, TILE, STRIP):
        bs = np.arange(width, n, width)
        lag_across[width] = [int(b) for b in bs if lag[b - 1] and lag[b]]
        live_across[width] = [int(b) for b in bs if pmin[b - 1] < min(1, g[b])]
    return dict(order=order, az=az_walk, chunks=chunks, T=T, lag=lag, lagging=int(lag.sum()), rises=rises,
                lag_across=lag_across, live_across=live_across)


# ---- clouds ------------------------------------------------------------------------------------------------------------------
def check_distinct(pts):
    az = azimuths(pts)
    assert np.unique(az).size == az.size, "azimuths tie: std::sort's order would not be the only one"
    assert not (az == 0.0).any(), "an azimuth of +-0.0: the two zeros compare equal"
    return az


def cloud_from_azimuths(az, seed, z_zero=False):
    """x = r cos a, y = r sin a with r in [4, 60) and z in [-2, 2) from a seeded generator (z = 0 on request: the CPU pin reads
    the chunk out of the oracle's z).  Asserts that the math.atan2 values of the result are pairwise distinct and not zero."""
    az = np.asarray(az, dtype=np.float64)
    rng = np.random.default_rng(seed)
    r = rng.uniform(4.0, 60.0, az.size)
    z = np.zeros(az.size) if z_zero else rng.uniform(-2.0, 2.0, az.size)
    pts = np.stack([r * np.cos(az), r * np.sin(az), z], axis=1)
    pts = pts[rng.permutation(az.size)]                 # (the input order is not the azimuth order)
    check_distinct(pts)
    return np.ascontiguousarray(pts)


SPARSE_SIZES = [1, 2, 37, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097]
SPARSE_KINDS = ["uniform", "sectors", "narrow", "bursts"]


def sparse_azimuths(kind, n, seed=0):
    rng = np.random.default_rng([seed, n, SPARSE_KINDS.index(kind)])
    if kind == "uniform":
        return rng.uniform(-math.pi, math.pi, n)
    if kind == "sectors":                               # three sectors with wide gaps between them
        w = rng.integers(3, size=n)
        return rng.uniform(np.array([-3.0, -0.4, 1.9])[w], np.array([-2.2, 0.5, 2.6])[w])
    if kind == "narrow":                                # one 0.2-rad sector (a limited-FOV sensor)
        return rng.uniform(-2.9, -2.7, n)
    if kind == "bursts":                                # 30 bursts 0.2 rad apart
        return -3.0 + 0.2 * rng.integers(30, size=n) + rng.uniform(0.0, 0.002, n)
    raise ValueError(kind)


def sparse_has_rise(kind, n):
    """Whether T_d - d rises anywhere in sparse_cloud(kind, n): it takes two neighbours at least two thresholds apart.  Not with
    one point, and not in the 0.2-rad sector (33 thresholds) once it holds many points per threshold or only two points: that
    family lags all the same — k_d = d + 1 from the first point on, about 960 thresholds behind — and holds the clamp
    min(1, .) rather than the carries."""
    return n >= 2 and not (kind == "narrow" and (n == 2 or n >= 255))


def sparse_cloud(kind, n, z_zero=False):
    return cloud_from_azimuths(sparse_azimuths(kind, n), seed=1000 + n, z_zero=z_zero)


STRADDLE_HEADS = {54: WAVE, 724: TILE, 1024: TILE, 3071: TILE, 261844: STRIP}  # head size -> the carry it is named for


def straddle_cloud(P, z_zero=False):
    """A dense head of P points in (pi - 0.5, pi - 0.001), a gap of about 600 thresholds, then 5 000 points in [-3.0, -2.9]: the
    walk lags for about 900 positions from P on (from 0 on for P = 54, whose head is itself sparse)."""
    rng = np.random.default_rng([7, P])
    az = np.concatenate([rng.uniform(math.pi - 0.5, math.pi - 0.001, P), rng.uniform(-3.0, -2.9, 5000)])
    return cloud_from_azimuths(az, seed=2000 + P % 1000, z_zero=z_zero)


def table_end_clouds(z_zero=False):
    """name -> cloud, at the end of the threshold table."""
    rng = np.random.default_rng(11)
    out = {}
    # azimuths in (-pi, -pi + 3 resolution) only: the walk never catches up, k_d = d + 1
    out["last_three_chunks"] = cloud_from_azimuths(rng.uniform(-math.pi + 1e-9, -math.pi + 3 * RESOLUTION, 300), 3001, z_zero)
    for name, y0 in (("minus_pi", -0.0), ("plus_pi", 0.0)):  # atan2(-+0.0, x < 0) = -+pi exactly; one such point only
        pts = cloud_from_azimuths(rng.uniform(-math.pi + 1e-9, math.pi - 1e-9, 1500), 3002, z_zero)
        pts[700] = [-17.25, y0, 0.0 if z_zero else 0.5]
        az = check_distinct(pts)
        assert az[700] == (-math.pi if name == "minus_pi" else math.pi)
        out[name] = pts
    return out


def _near(target_lo, target_hi, thr, rng):
    """(x, y) whose libm azimuth a satisfies target_lo <= |a - thr| <= target_hi on the side given by the signs (both bounds
    carry the side's sign), found by search."""
    for _ in range(200):
        off = rng.uniform(min(target_lo, target_hi), max(target_lo, target_hi))
        r = rng.uniform(4.0, 60.0)
        x, y = r * math.cos(thr + off), r * math.sin(thr + off)
        a = math.atan2(y, x)
        if min(target_lo, target_hi) <= a - thr <= max(target_lo, target_hi) and a != thr:
            return x, y
    raise AssertionError("no point found near threshold %r" % thr)


def near_threshold_cloud(lo=1e-12, hi=1e-10, every=5, background=3, z_zero=False):
    """About 2 * 1023 / every points whose libm azimuth lies between `lo` and `hi` rad BELOW / ABOVE every `every`-th threshold, in
    a background of `background` points strictly inside every threshold interval — dense enough for the walk to have caught up
    where the near points sit, so that their chunk is decided by their side of the threshold and by nothing else.
    Returns (cloud, mask of the near points)."""
    rng = np.random.default_rng(13)
    thr = thresholds(CHUNKS - 1)                        # the thresholds above -pi
    xy, near = [], []
    for k in range(0, thr.size - 1):
        a = rng.uniform(thr[k + 1] + 0.25 * RESOLUTION, thr[k] - 0.25 * RESOLUTION, background)
        r = rng.uniform(4.0, 60.0, background)
        xy += list(zip(r * np.cos(a), r * np.sin(a)))
        near += [False] * background
    for k in range(2, thr.size - 1, every):
        for sign in (-1.0, 1.0):
            xy.append(_near(sign * lo, sign * hi, thr[k], rng))
            near.append(True)
    xy, near = np.array(xy), np.array(near)
    z = np.zeros(len(xy)) if z_zero else rng.uniform(-2.0, 2.0, len(xy))
    pts = np.column_stack([xy, z])
    perm = rng.permutation(len(pts))
    pts, near = np.ascontiguousarray(pts[perm]), near[perm]
    az = check_distinct(pts)
    dist = np.abs(az[near, None] - thr[None, :]).min(axis=1)
    assert (dist >= lo).all() and (dist <= hi).all(), (dist.min(), dist.max())
    return pts, near


def on_threshold_points(count=60, tries=4000):
    """Points whose libm azimuth EQUALS a threshold, found by stepping y through neighbouring doubles (not every threshold
    has one within reach: returns what it finds).  For the census only."""
    rng = np.random.default_rng(17)
    thr = thresholds(CHUNKS - 1)
    out = []
    for k in rng.permutation(thr.size - 2)[:count] + 1:
        t = float(thr[k])
        r = rng.uniform(4.0, 60.0)
        x, y = r * math.cos(t), r * math.sin(t)
        for _ in range(tries):
            a = math.atan2(y, x)
            if a == t:
                out.append((x, y))
                break
            y = math.nextafter(y, math.inf if (a < t) == (x > 0) else -math.inf)
    return np.array(out).reshape(-1, 2)
