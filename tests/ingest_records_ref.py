"""A plain numpy restatement of madicp_cloud_ingest_records (include/madicp_hip.h) / madicp_host_ingest_records, and the
layouts, counts and time families that try them.

TEST INFRASTRUCTURE ONLY.  The rules, all fp64:

    survivors   the keep mask of oracle_lib.ingest_f32 on the three floats at off_x / off_y / off_z: float norm
                sqrt(x*x + (y*y + z*z)) compared in double, ON a bound stays, NaN coordinates dropped; the coordinates ARE
                oracle_lib.ingest_f32's for the (n, 3) float32 view (its row count must equal this module's own mask count)
    time        t64 = float64(field): exact for uint32, float32, float64
    range       automatic: min / max of t64 over ALL records with a finite time (dropped ones included), each + 0.0;
                (+inf, -inf) when there is none.  explicit: as given
    stamp       (t64 - t0) / (t1 - t0); all NaN unless t1 - t0 > 0

  LAYOUTS            the nine record layouts, as mad_icp_amd.records.RecordLayout tuples
  pack(...)          a byte buffer of one layout: junk bytes everywhere, then the fields
  fields(buf, lay)   the (n, 3) float32 coordinates and the float64 times read back out of a buffer (unaligned structured view)
  reference(...)     (points, stamps or None, (t0, t1))
  time families      TIME_FAMILIES: name -> f(n, keep, rng) -> (times in the field's dtype, t_type)
"""
import numpy as np

import oracle_lib as O
from mad_icp_amd.records import T_F32, T_F64, T_NONE, T_U32, RecordLayout

LO, HI = 0.7, 120.0

LAYOUTS = {
    "xyz12": RecordLayout(12, 0, 4, 8, 0, T_NONE),        # xyz only
    "odd13": RecordLayout(13, 1, 5, 9, 0, T_NONE),        # every record at another alignment
    "kitti16": RecordLayout(16, 0, 4, 8, 12, T_F32),      # time = the 4th float
    "xyzirt22": RecordLayout(22, 0, 4, 8, 18, T_F32),     # packed XYZIRT
    "f64at18": RecordLayout(26, 0, 4, 8, 18, T_F64),      # never 8-aligned
    "reversed32": RecordLayout(32, 8, 4, 0, 24, T_F64),   # z, y, x in reversed offsets
    "ouster48": RecordLayout(48, 0, 4, 8, 20, T_U32),
    "tail255": RecordLayout(255, 0, 4, 8, 251, T_U32),    # the last bytes of the record
    "cap256": RecordLayout(256, 0, 4, 8, 248, T_F64),     # the cap
}
COUNTS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 4096]
PATTERNS = ("all", "first", "last", "alternating", "one_per_tile")
TIME_DTYPE = {T_U32: "<u4", T_F32: "<f4", T_F64: "<f8"}


def survivors(pattern, n):
    """the survivor patterns of tests/test_gpu_frontend_edges.py"""
    keep = np.zeros(n, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "alternating":
        keep[::2] = True
    else:  # one per tile of 1024 marks, at another place in every tile
        t = np.arange((n + 1023) // 1024)
        keep[np.minimum(t * 1024 + (37 * t + 5) % 1024, n - 1)] = True
    return keep


def patterned(keep, seed):
    """float32 coordinates kept where `keep`, dropped elsewhere (below LO and beyond HI in turn)"""
    rng = np.random.default_rng(seed)
    n = keep.size
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz = d * rng.uniform(2.0, 60.0, n)[:, None]
    drop = d * np.where(np.arange(n) % 2 == 0, 0.3, 300.0)[:, None]
    return np.where(keep[:, None], xyz, drop).astype(np.float32)


def view_dtype(lay):
    names, formats, offsets = ["x", "y", "z"], ["<f4"] * 3, [lay.off_x, lay.off_y, lay.off_z]
    if lay.t_type != T_NONE:
        names.append("t")
        formats.append(TIME_DTYPE[lay.t_type])
        offsets.append(lay.off_t)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=lay.point_step))


def pack(lay, xyz32, times=None, seed=0):
    """(n, point_step) uint8: random bytes in every other field, then x / y / z (and the times, given in the field's dtype)"""
    n = xyz32.shape[0]
    buf = np.random.default_rng([seed, lay.point_step]).integers(0, 256, size=(n, lay.point_step), dtype=np.uint8)
    v = buf.reshape(-1).view(view_dtype(lay))
    v["x"], v["y"], v["z"] = xyz32[:, 0], xyz32[:, 1], xyz32[:, 2]
    if lay.t_type != T_NONE:
        assert times is not None and times.dtype == np.dtype(TIME_DTYPE[lay.t_type])
        v["t"] = times
    return buf


def fields(buf, lay):
    v = np.ascontiguousarray(buf).reshape(-1).view(view_dtype(lay))
    xyz = np.stack([np.array(v["x"]), np.array(v["y"]), np.array(v["z"])], axis=1)
    t64 = np.array(v["t"]).astype(np.float64) if lay.t_type != T_NONE else None
    return xyz, t64


def time_range(t64):
    fin = t64[np.isfinite(t64)]
    if fin.size == 0:
        return np.inf, -np.inf
    return float(fin.min() + 0.0), float(fin.max() + 0.0)


def reference(buf, lay, lo, hi, kitti, t_range=None):
    xyz, t64 = fields(buf, lay)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        nrm = np.sqrt(x * x + (y * y + z * z)).astype(np.float64)
        keep = ~((nrm < lo) | (nrm > hi) | np.isnan(x) | np.isnan(y) | np.isnan(z))
        pts = O.ingest_f32(xyz, lo, hi, kitti)
    assert int(keep.sum()) == pts.shape[0]
    if t64 is None:
        return pts, None, (np.inf, -np.inf)
    t0, t1 = time_range(t64) if t_range is None else (float(t_range[0]), float(t_range[1]))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        span = np.float64(t1) - np.float64(t0)
        s = (t64 - t0) / span if span > 0 else np.full(t64.shape, np.nan)
    return pts, s[keep], (t0, t1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """equal shapes, NaN at the same places, everything else bit for bit (the sign of a zero counts)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


# ---- time families: f(n, keep, rng) -> times in the dtype of the family's field type -----------------------------------------------
def _u32_ns(n, keep, rng):
    """nanoseconds 0 .. 1e8, the minimum in the LAST record and the maximum in the FIRST"""
    t = rng.integers(1, 10**8, size=n).astype("<u4")
    t[-1], t[0] = 0, 10**8
    if n == 1:
        t[0] = 5
    return t


def _u32_extremes_dropped(n, keep, rng):
    """the same with both extremes in DROPPED records (the first lane of the first tile, the last record of the last tile) where
    the pattern drops them: the range still comes from the whole message"""
    t = rng.integers(1000, 10**8 - 1000, size=n).astype("<u4")
    t[0], t[-1] = 10**8, 0
    return t


def _equal(n, keep, rng):
    return np.full(n, 12345.5, "<f4")


def _f32_specials(n, keep, rng):
    t = rng.uniform(0.0, 0.1, n).astype("<f4")
    t[rng.integers(n, size=max(1, n // 7))] = np.nan
    t[rng.integers(n, size=max(1, n // 11))] = np.inf
    t[rng.integers(n, size=max(1, n // 13))] = -np.inf
    return t


def _f32_signed_zero_min(n, keep, rng):
    """both +0.0 and -0.0 as the minimum: t0 must come out +0.0 whichever a reduction meets first"""
    t = rng.uniform(0.01, 0.1, n).astype("<f4")
    t[rng.integers(n, size=max(1, n // 5))] = 0.0
    t[rng.integers(n, size=max(1, n // 5))] = -0.0
    t[n // 2] = -0.0
    if n > 1:
        t[n // 2 - 1] = 0.0
    return t


def _f64_epoch(n, keep, rng):
    return (1.7e9 + rng.uniform(0.0, 0.1, n)).astype("<f8")


TIME_FAMILIES = {
    "u32_ns": (_u32_ns, T_U32),
    "u32_extremes_dropped": (_u32_extremes_dropped, T_U32),
    "equal": (_equal, T_F32),
    "f32_specials": (_f32_specials, T_F32),
    "f32_signed_zero_min": (_f32_signed_zero_min, T_F32),
    "f64_epoch": (_f64_epoch, T_F64),
}
# a layout of every field type, for the families
FAMILY_LAYOUT = {T_U32: ("ouster48", "tail255"), T_F32: ("xyzirt22", "kitti16"), T_F64: ("f64at18", "cap256")}


def generic_times(lay, n, seed):
    """plain times of the layout's type for the cases that are about something else"""
    rng = np.random.default_rng([seed, 77])
    if lay.t_type == T_U32:
        return rng.integers(0, 10**8, size=n).astype("<u4")
    if lay.t_type == T_F32:
        return rng.uniform(0.0, 0.1, n).astype("<f4")
    if lay.t_type == T_F64:
        return (1.7e9 + rng.uniform(0.0, 0.1, n)).astype("<f8")
    return None
