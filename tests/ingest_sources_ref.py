"""A plain numpy restatement of madicp_cloud_ingest_sources (include/madicp_hip.h) / madicp_host_ingest_sources, and the case
table that tries them.

TEST INFRASTRUCTURE ONLY.  Per source, tests/ingest_records_ref.py's rules (the survivors and their coordinates, the time as a
float64) with that source's OWN range bounds in its own frame, then, all fp64 with numpy's separate `*` and `+` (two roundings):

    common clock    tc = t64 * t_scale + t_offset; t64 itself when t_scale == 1.0 and t_offset == 0.0 exactly
    range           automatic: min / max of tc over ALL records of ALL sources with a finite tc, each + 0.0; (+inf, -inf) when
                    there is none or no time field.  explicit: as given
    stamp           (tc - t0) / (t1 - t0); all NaN unless t1 - t0 > 0
    sensor -> base  after the optional KITTI rotation: base[i] = t[i] + (R[i,0] * o0 + (R[i,1] * o1 + R[i,2] * o2)); skipped when
                    sensor_to_base is exactly the identity
    order           source 0's survivors in input order, then source 1's ...

  reference(sources, t_range)   (points, stamps or None, (t0, t1), survivors per source)
  CASES                         name -> f() -> (sources, t_range): the shapes at which the tile and source bookkeeping can go wrong
  reassembly(...)               a scan split into an identity source and a rotated, time-shifted one that must merge back exactly
  bad_source_sets()             what both native entries refuse; native_args(...) builds the C arguments of any of them
"""
import copy

import numpy as np

import ingest_records_ref as R
from mad_icp_amd import capi
from mad_icp_amd.records import T_F32, T_F64, T_NONE, T_U32, RecordLayout, Source

LO, HI = R.LO, R.HI


def per_tile(step):
    return 256 if step <= 64 else (128 if step <= 128 else 64)


def _extrinsic(src):
    return np.eye(4) if src.sensor_to_base is None else np.asarray(src.sensor_to_base, dtype=np.float64)


def reference(sources, t_range=None):
    pts_all, tc_all, keep_all, per = [], [], [], []
    timed = RecordLayout(*sources[0].layout).t_type != T_NONE
    for src in sources:
        lay = RecordLayout(*src.layout)
        xyz, t64 = R.fields(src.records, lay)
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            nrm = np.sqrt(x * x + (y * y + z * z)).astype(np.float64)
            keep = ~((nrm < src.min_range) | (nrm > src.max_range) | np.isnan(x) | np.isnan(y) | np.isnan(z))
            pts, _, _ = R.reference(src.records, lay._replace(off_t=0, t_type=T_NONE), src.min_range, src.max_range,
                                    int(bool(src.kitti_correction)))
        assert pts.shape[0] == int(keep.sum())
        T = _extrinsic(src)
        if not np.array_equal(T[:3], np.eye(4)[:3]):
            Rm, t = T[:3, :3], T[:3, 3]
            o0, o1, o2 = pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()
            with np.errstate(over="ignore", invalid="ignore"):
                pts = np.stack([t[i] + (Rm[i, 0] * o0 + (Rm[i, 1] * o1 + Rm[i, 2] * o2)) for i in range(3)], axis=1)
        pts_all.append(pts)
        per.append(pts.shape[0])
        keep_all.append(keep)
        if timed:
            scale, offset = np.float64(src.time_scale), np.float64(src.time_offset)
            with np.errstate(over="ignore", invalid="ignore"):
                tc_all.append(t64 if (scale == 1.0 and offset == 0.0) else t64 * scale + offset)
    pts = np.concatenate(pts_all, axis=0)
    if not timed:
        return pts, None, (np.inf, -np.inf), per
    tc, keep = np.concatenate(tc_all), np.concatenate(keep_all)
    t0, t1 = R.time_range(tc) if t_range is None else (float(t_range[0]), float(t_range[1]))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        span = np.float64(t1) - np.float64(t0)
        s = (tc - t0) / span if span > 0 else np.full(tc.shape, np.nan)
    return pts, s[keep], (t0, t1), per


# ---- sources for the case table ------------------------------------------------------------------------------------------------------
def rigid(seed):
    """a general rotation (QR of a random matrix, det +1) and translation: 4x4"""
    rng = np.random.default_rng([seed, 5])
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Q, rng.uniform(-2.0, 2.0, 3)
    return T


def seconds_as(lay, seconds):
    """times of a frame (seconds from its start) in the layout's field type: uint32 nanoseconds, float32 / float64 seconds"""
    if lay.t_type == T_U32:
        return np.round(seconds * 1e9).astype("<u4")
    return None if lay.t_type == T_NONE else seconds.astype(R.TIME_DTYPE[lay.t_type])


def source(lay, n, seed, keep=None, times=None, lo=LO, hi=HI, **kw):
    """a Source of n records of one layout: about one record in five dropped (tests/ingest_records_ref.patterned) unless `keep`
    says otherwise, times 0 .. 0.1 s in the field's units unless given; uint32 fields get time_scale = 1e-9 unless given"""
    lay = RecordLayout(*lay)
    rng = np.random.default_rng([seed, n, lay.point_step])
    if keep is None:
        keep = rng.integers(5, size=n) != 0
    if times is None:
        times = seconds_as(lay, rng.uniform(0.0, 0.1, n))
    if lay.t_type == T_U32:
        kw.setdefault("time_scale", 1e-9)
    return Source(R.pack(lay, R.patterned(keep, seed), times, seed=seed), lo, hi, layout=lay, **kw)


L16, L22 = RecordLayout(16, 0, 4, 8, 12, T_F32), RecordLayout(22, 0, 4, 8, 18, T_U32)
# the eight steps of case E: all three tile sizes, the time types mixed at odd offsets
E_LAYOUTS = [L16, L22, RecordLayout(26, 0, 4, 8, 17, T_F64), RecordLayout(48, 0, 4, 8, 21, T_U32), RecordLayout(65, 1, 5, 9, 33, T_F32),
             RecordLayout(129, 3, 7, 11, 57, T_F64), RecordLayout(200, 0, 4, 8, 101, T_U32), RecordLayout(256, 0, 4, 8, 247, T_F64)]


def case_a():
    rng = np.random.default_rng(1)
    times = rng.integers(0, 10**8, size=1000).astype("<u4")
    return [source(L22, 1000, 1, times=times, time_scale=1.0)], None


def case_b():
    return [source(L16, 256, 2), source(L22, 257, 3, time_offset=0.01)], None


def case_c():
    keep = np.ones(1, bool)
    return [source(L16, 1, 4, keep=keep, times=np.array([0.02], "<f4")),
            source((20, 0, 4, 8, 16, T_U32), 1, 5, keep=keep, times=np.array([5 * 10**7], "<u4"), sensor_to_base=rigid(5)),
            source((28, 0, 4, 8, 20, T_F64), 1, 6, keep=keep, times=np.array([0.09], "<f8"), time_offset=-0.005)], None


def case_d():
    return [source((13, 1, 5, 9, 0, T_NONE), 37, 7), source((12, 0, 4, 8, 0, T_NONE), 5, 8, sensor_to_base=rigid(8)),
            source((255, 0, 4, 8, 0, T_NONE), 3, 9, keep=np.array([True, False, True]))], None


def case_e():
    return [source(lay, 2 * per_tile(lay.point_step) + 3, 10 + k, time_offset=0.001 * k, sensor_to_base=rigid(10 + k) if k % 2 else None)
            for k, lay in enumerate(E_LAYOUTS)], None


def case_f():
    """source 0: every record beyond max_range, its times hold the global minimum"""
    n = 300
    early = source(L22, n, 20, keep=np.zeros(n, bool), times=np.arange(n, dtype="<u4") * 1000)
    late = source(L16, 400, 21, times=np.random.default_rng(21).uniform(0.05, 0.1, 400).astype("<f4"))
    return [early, late], None


def case_g():
    return [source(L22, 300, 22, keep=np.zeros(300, bool)), source(L16, 257, 23, keep=np.zeros(257, bool))], None


def case_h():
    """non-finite times in one source, every finite time equal on the common clock: no span, all stamps NaN"""
    n = 300
    t = np.full(n, 5.0, "<f4")
    t[::7], t[3::11], t[5::13] = np.nan, np.inf, -np.inf
    return [source(L16, n, 24, times=t), source(L22, 257, 25, times=np.full(257, 5, "<u4"), time_scale=1.0)], None


def case_i():
    return [source(L16, 500, 26), source(L22, 300, 27, time_offset=0.02)], (0.03, 0.06)


def case_j():
    """uint32 nanoseconds from two message headers 1.25 ms apart, float64 seconds already on the common clock"""
    rng = np.random.default_rng(28)
    return [source(L22, 700, 28, time_offset=0.0), source((48, 0, 4, 8, 21, T_U32), 513, 29, time_offset=0.00125),
            source((26, 0, 4, 8, 17, T_F64), 300, 30, times=rng.uniform(0.0, 0.1, 300).astype("<f8"))], None


def case_k():
    return [source(L22, 600, 31, kitti_correction=True, sensor_to_base=rigid(31), lo=1.0, hi=50.0),
            source(L16, 515, 32, kitti_correction=False, sensor_to_base=rigid(32), lo=3.0, hi=90.0)], None


def case_m():
    """more tiles (4 097 of 64 records, + 1) than any grid the launch rule can pick: a second trip of the grid-stride loop"""
    return [source((136, 0, 4, 8, 100, T_F64), 64 * 4096 + 5, 33, sensor_to_base=rigid(33)), source(L22, 100, 34, time_offset=0.003)], None


CASES = {"A": case_a, "B": case_b, "C": case_c, "D": case_d, "E": case_e, "F": case_f, "G": case_g, "H": case_h, "I": case_i,
         "J": case_j, "K": case_k, "M": case_m}


# ---- exact reassembly (case L) ---------------------------------------------------------------------------------------------------------
RZ90 = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]])  # exact in float32
TIME_SHIFT = 4096


def quantised(scan, lo=LO, hi=HI):
    """a scan's coordinates as multiples of 2^-8 (zeros canonicalised) in float32, without the points whose range lies within
    1.5 m of a bound: the filter runs in each SENSOR's frame, 1.15 m from the base's, and must decide the same in both"""
    q = (np.round(np.asarray(scan, np.float64) * 256.0) / 256.0 + 0.0).astype(np.float32)
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    return np.ascontiguousarray(q[(r > lo + 1.5) & (r < hi - 1.5)])


def reassembly(xyz32, ticks, lay=L22, lo=LO, hi=HI):
    """(unsplit records (n, step) uint8, [identity source of the first half, rotated and time-shifted source of the second]) of
    quantised base-frame points and uint32 times >= TIME_SHIFT.  Every operation of the split and of the merge is exact."""
    n = xyz32.shape[0]
    h = n // 2
    assert ticks.dtype == np.dtype("<u4") and ticks.min() >= TIME_SHIFT
    whole = R.pack(lay, xyz32, ticks, seed=77)
    Rm, t = RZ90[:3, :3], RZ90[:3, 3]
    sensor = ((xyz32[h:].astype(np.float64) - t) @ Rm).astype(np.float32)              # R^T (p - t), exact
    assert np.array_equal(sensor.astype(np.float64) @ Rm.T + t, xyz32[h:].astype(np.float64))
    first = Source(R.pack(lay, xyz32[:h], ticks[:h], seed=78), lo, hi, layout=lay)
    second = Source(R.pack(lay, sensor, ticks[h:] - np.uint32(TIME_SHIFT), seed=79), lo, hi, layout=lay, sensor_to_base=RZ90,
                    time_offset=float(TIME_SHIFT))
    return whole, [first, second]


# ---- what the native entries refuse ----------------------------------------------------------------------------------------------------
def native_args(sources, t_range):
    """(arrays kept alive, RecordSourceC array, n_sources, t_range array or None) of a call.  The string "HUGE" among the sources
    stands for the one case no array can be built for: a copy of the first source that claims 2^30 records."""
    real = [s for s in sources if not isinstance(s, str)]
    if "HUGE" in sources:
        real = real + [copy.copy(real[0])]
    alive, arr, _, _, tr = capi._sources_args(real, t_range)
    if "HUGE" in sources:
        arr[len(real) - 1].n_records = 2**30
    return alive, arr, len(real), tr


def bad_source_sets():
    """(why, sources, t_range) of everything both native entries refuse: shared with tests/test_gpu_ingest_sources.py"""
    good = lambda seed=60, **kw: source(L22, 300, seed, **kw)  # noqa: E731
    out = [("no source", [], None), ("nine sources", [good(60 + k) for k in range(9)], None)]
    empty = good()
    empty.records = empty.records[:0]
    out.append(("an empty source", [good(), empty], None))
    huge = good()
    out.append(("more than 2^30 records in all", [huge, "HUGE"], None))
    for bad in [(11, 0, 4, 7, 0, 0), (257, 0, 4, 8, 0, 0), (22, -1, 4, 8, 18, 7), (22, 0, 19, 8, 18, 7), (22, 0, 4, 8, 19, 7),
                (22, 0, 4, 8, 15, 8), (22, 0, 4, 8, 18, 5)]:
        s = good()
        s.layout = bad
        out.append(("layout %r" % (bad,), [good(61), s], None))
    for where in [(0, 0), (2, 1), (1, 3), (2, 3)]:
        for v in (np.nan, np.inf):
            T = rigid(3)
            T[where] = v
            out.append(("sensor_to_base[%d,%d] = %r" % (where + (v,)), [good(sensor_to_base=T)], None))
    for scale in (0.0, -1e-9, np.nan, np.inf):
        out.append(("time_scale %r" % scale, [good(61), good(time_scale=scale)], None))
    for offset in (np.nan, np.inf, -np.inf):
        out.append(("time_offset %r" % offset, [good(time_offset=offset)], None))
    out.append(("with and without a time field", [good(), source((13, 1, 5, 9, 0, T_NONE), 37, 62)], None))
    out.append(("without and with a time field", [source((13, 1, 5, 9, 0, T_NONE), 37, 62), good()], None))
    for tr in [(2.0, 1.0), (1.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (-np.inf, 0.0)]:
        out.append(("t_range %r" % (tr,), [good()], tr))
    return out
