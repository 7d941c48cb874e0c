"""The export rule of include/madicp_hip.h (madicp_cloud_export_f32) restated in numpy, and the input sets the host and the
device tests share.  Everything in float64, elementwise (numpy does not fuse):
  position  q[i] = t[i] + (R[3i] p0 + (R[3i+1] p1 + R[3i+2] p2))
  output    float32(q), round to nearest even
  voxel 0   every point, cloud order
  voxel >0  cell = floor(q / voxel) per axis; candidate iff -2^20 <= cell < 2^20 on all three (NaN / inf fail); key = (kx + 2^20) |
            (ky + 2^20) << 21 | (kz + 2^20) << 42; the lowest index of every key, ascending index order."""
import numpy as np

CELL = 1048576.0


def positions(xyz, R, t):
    p = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    q = np.empty_like(p)
    with np.errstate(all="ignore"):
        for i in range(3):
            a, b, c = R[i, 0] * p[:, 0], R[i, 1] * p[:, 1], R[i, 2] * p[:, 2]
            q[:, i] = t[i] + (a + (b + c))
    return q


def kept_indices(q, voxel):
    """indices (ascending) of the rows that go out"""
    n = q.shape[0]
    if voxel == 0:
        return np.arange(n)
    with np.errstate(all="ignore"):
        f = np.floor(q / voxel)
        cand = np.all((f >= -CELL) & (f < CELL), axis=1)
    idx = np.nonzero(cand)[0]
    if idx.size == 0:
        return idx
    k = f[idx].astype(np.int64) + int(CELL)
    key = k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)
    _, first = np.unique(key, return_index=True)  # (the first occurrence of every key: idx ascends)
    return np.sort(idx[first])


def export_f32(xyz, R, t, voxel):
    q = positions(xyz, R, t)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(q[kept_indices(q, voxel)].astype(np.float32))


def same_bits(a, b):
    """float32 arrays equal bit for bit, compared as uint32 — after every NaN has been replaced by ONE quiet NaN: IEEE 754 leaves
    the sign and payload of a NaN that an operation produces or passes on to the implementation (x86 hands on its first operand's,
    and a compiler may commute an addition; 0 * inf gives the negative default NaN there, numpy's constant is the positive one),
    so they are no part of the rule.  -0.0 and +0.0, and every other value, must match exactly."""
    a, b = np.array(a, dtype=np.float32, copy=True), np.array(b, dtype=np.float32, copy=True)
    if a.shape != b.shape:
        return False
    a[np.isnan(a)] = np.float32(np.nan)
    b[np.isnan(b)] = np.float32(np.nan)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


IDENTITY = (np.eye(3), np.zeros(3))


def random_pose(seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(3, 3))
    Q, _ = np.linalg.qr(A)
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return np.ascontiguousarray(Q), rng.normal(size=3) * 5.0


def gaussian(n, seed, scale=8.0):
    return np.random.default_rng(seed).normal(size=(n, 3)) * scale


def on_faces(n, seed):
    """coordinates that are multiples of 0.5 (cell faces at voxel 0.5), negative ones and -0.0 included, and -0.25 (cell -1)"""
    rng = np.random.default_rng(seed)
    p = rng.integers(-6, 7, size=(n, 3)).astype(np.float64) * 0.5
    p[::5, 0] = -0.0
    p[1::7, 1] = -0.25
    return p


def duplicates(n, seed):
    base = gaussian(max(1, n // 3), seed)
    return base[np.random.default_rng(seed + 1).integers(0, base.shape[0], size=n)]


def one_cell(n, seed):
    """all points strictly inside the cell [0, 0.001)^3 ... of every voxel size used, under the identity"""
    return np.random.default_rng(seed).uniform(1e-5, 9e-4, size=(n, 3))


def own_cells(n):
    """every point in its own cell at any voxel <= 1: a 1.5-spaced lattice line folded into a cube"""
    i = np.arange(n)
    return np.stack([(i % 37) * 1.5 + 0.25, ((i // 37) % 37) * 1.5 + 0.25, (i // 1369) * 1.5 + 0.25], axis=1).astype(np.float64)


def two_cells(n):
    p = np.full((n, 3), 0.125)
    p[1::2, 0] = 7.125
    return p


def with_nonfinite(p, seed):
    p = np.array(p, dtype=np.float64, copy=True)
    n = p.shape[0]
    rng = np.random.default_rng(seed)
    for v in (np.nan, np.inf, -np.inf):
        rows = rng.integers(0, n, size=max(1, n // 9))
        p[rows, rng.integers(0, 3, size=rows.size)] = v
    return p


def range_edge(voxel):
    """under the identity: q = 2^20 * voxel is dropped (cell 2^20), q = -2^20 * voxel kept (cell -2^20), and the neighbours"""
    e = CELL * voxel
    return np.array([[e, 0.0, 0.0], [-e, 0.0, 0.0], [0.0, e, 0.0], [0.0, -e, 0.0], [0.0, 0.0, e], [0.0, 0.0, -e],
                     [np.nextafter(e, 0.0), 1.0 * voxel, 0.0], [np.nextafter(-e, -np.inf), 0.0, 0.0], [0.5 * voxel, 0.5 * voxel, 0.5 * voxel]])


def synthetic_scan(n_beams=16, n_azimuth=450, seed=3):
    """a 16 x 450 spinning-head scan of a box room: ranges 3 .. 25 m, in firing order"""
    rng = np.random.default_rng(seed)
    az = np.repeat(np.linspace(np.pi, -np.pi, n_azimuth, endpoint=False), n_beams)
    el = np.tile(np.deg2rad(np.linspace(-15.0, 15.0, n_beams)), n_azimuth)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    half = np.array([12.0, 7.0, 2.5])
    with np.errstate(divide="ignore"):
        r = np.min(half / np.abs(d), axis=1)
    r = r + rng.normal(size=r.shape) * 0.01
    return (d * r[:, None]).astype(np.float32).astype(np.float64)


def input_sets(n, seed):
    """(name, points) of the sets every size is checked on"""
    return [("gaussian", gaussian(n, seed)), ("faces", on_faces(n, seed + 1)), ("duplicates", duplicates(n, seed + 2)),
            ("one_cell", one_cell(n, seed + 3)), ("own_cells", own_cells(n)), ("two_cells", two_cells(n)),
            ("nonfinite", with_nonfinite(gaussian(n, seed + 4), seed + 5))]
