"""The host twin of the records ingest (madicp_host_ingest_records, csrc/host/ingest_records.cpp) against the numpy restatement of
tests/ingest_records_ref.py, bit for bit: every layout at every count and survivor pattern, every time family, explicit ranges,
the refusals, and the layout helper of mad_icp_amd.records.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ingest_records_ref as R
from mad_icp_amd import capi, records


def check(buf, lay, kitti, t_range=None, expect_kept=None):
    ref_p, ref_s, ref_r = R.reference(buf, lay, R.LO, R.HI, kitti, t_range)
    if expect_kept is not None:
        assert ref_p.shape[0] == expect_kept
    pts, st, rng = capi.host_ingest_records(buf, R.LO, R.HI, kitti, layout=lay, t_range=t_range)
    assert R.same_bits(pts, ref_p)
    assert R.same_bits(np.array(rng), np.array(ref_r)), (rng, ref_r)
    if lay.t_type == records.T_NONE:
        assert st is None
    else:
        assert R.same_bits(st, ref_s)
    return pts, st, rng


@pytest.mark.parametrize("kitti", [0, 1])
@pytest.mark.parametrize("name", sorted(R.LAYOUTS))
def test_layouts_counts_and_survivor_patterns(natives, name, kitti):
    lay = R.LAYOUTS[name]
    for n in R.COUNTS:
        for pattern in R.PATTERNS:
            keep = R.survivors(pattern, n)
            xyz = R.patterned(keep, n)
            buf = R.pack(lay, xyz, R.generic_times(lay, n, n), seed=n)
            pts, _, _ = check(buf, lay, kitti, expect_kept=int(keep.sum()))
            if not kitti:
                assert np.array_equal(pts, xyz[keep].astype(np.float64)), (n, pattern)


@pytest.mark.parametrize("family", sorted(R.TIME_FAMILIES))
def test_time_families(natives, family):
    make, t_type = R.TIME_FAMILIES[family]
    for name in R.FAMILY_LAYOUT[t_type]:
        lay = R.LAYOUTS[name]
        for n in (1, 2, 257, 1025, 4096):
            for pattern in ("all", "alternating", "one_per_tile"):
                keep = R.survivors(pattern, n)
                if family == "u32_extremes_dropped" and n > 2:
                    keep[0] = keep[-1] = False
                    keep[1] = True
                times = make(n, keep, np.random.default_rng([n, 3]))
                buf = R.pack(lay, R.patterned(keep, n), times, seed=n)
                _, st, rng = check(buf, lay, 0, expect_kept=int(keep.sum()))
                if family == "equal" or n == 1:
                    assert np.isnan(st).all()
                if family == "u32_extremes_dropped" and n > 2:
                    assert rng == (0.0, 1e8) and st.min() > 0.0 and st.max() < 1.0
                if family == "f32_signed_zero_min" and n > 1:
                    assert rng[0] == 0.0 and not np.signbit(rng[0])
                if family == "u32_ns" and n > 1:
                    assert rng == (0.0, 1e8)


def test_explicit_range_narrower_than_the_data(natives):
    lay = R.LAYOUTS["f64at18"]
    n = 1025
    keep = R.survivors("alternating", n)
    times = R.generic_times(lay, n, 5)
    buf = R.pack(lay, R.patterned(keep, 5), times, seed=5)
    tr = (1.7e9 + 0.03, 1.7e9 + 0.06)
    _, st, rng = check(buf, lay, 1, t_range=tr)
    assert rng == tr and st.min() < 0.0 and st.max() > 1.0


def test_refusals(natives):
    L = capi.host_lib()
    lay = R.LAYOUTS["xyzirt22"]
    n = 10
    buf = R.pack(lay, R.patterned(np.ones(n, bool), 1), R.generic_times(lay, n, 1))
    xyz, st, kept = np.empty((n, 3)), np.empty(n), C.c_int64(-7)
    dp = C.POINTER(C.c_double)

    def call(layout, count=n, data=buf.ctypes.data_as(C.c_void_p), t_range=None, out=xyz.ctypes.data_as(dp), lay_null=False):
        cl = capi.RecordLayoutC(*layout)
        tr = None if t_range is None else np.array(t_range, np.float64)
        return L.madicp_host_ingest_records(data, count, None if lay_null else C.byref(cl), R.LO, R.HI, 0,
                                            None if tr is None else tr.ctypes.data_as(dp), out, st.ctypes.data_as(dp), C.byref(kept), None)

    assert call(lay) == 0 and kept.value == n
    kept.value = -7
    assert call(lay, data=None) == -1 and call(lay, out=None) == -1 and call(lay, lay_null=True) == -1
    assert call(lay, count=0) == -1 and call(lay, count=-1) == -1 and call(lay, count=2**30 + 1) == -1
    assert call(lay, count=2**30) == -1              # this entry's own bound: the sources rule would allow it
    for bad in [(11, 0, 4, 7, 0, 0), (257, 0, 4, 8, 0, 0), (22, -1, 4, 8, 18, 7), (22, 0, 19, 8, 18, 7), (22, 0, 4, 22, 18, 7),
                (22, 0, 4, 8, 19, 7), (22, 0, 4, 8, 15, 8), (22, 0, 4, 8, -1, 6), (22, 0, 4, 8, 18, 5), (22, 0, 4, 8, 18, 9)]:
        assert call(bad) == -1, bad
    assert call((22, 0, 4, 8, 99, 0)) == 0          # off_t is ignored without a time field
    kept.value = -7
    for tr in [(2.0, 1.0), (1.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (-np.inf, 0.0)]:
        assert call(lay, t_range=tr) == -1, tr
    assert kept.value == -7                          # nothing written by a refusal
    # no survivor is not an error on the host: zero rows
    far = R.pack(lay, np.full((n, 3), 500.0, np.float32), R.generic_times(lay, n, 1))
    pts, stamps, _ = capi.host_ingest_records(far, R.LO, R.HI, 0, layout=lay)
    assert pts.shape == (0, 3) and stamps.shape == (0,)


def test_layout_helper(natives):
    T = records
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("ring", "<u2"), ("time", "<f4")])
    assert T.layout_of(dt) == T.RecordLayout(22, 0, 4, 8, 18, T.T_F32)
    assert T.layout_of(np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])) == T.RecordLayout(12, 0, 4, 8, 0, T.T_NONE)
    both = np.dtype([("timestamp", "<f8"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<u4")])
    assert T.layout_of(both) == T.RecordLayout(24, 8, 12, 16, 20, T.T_U32)                 # `t` comes first in the search order
    assert T.layout_of(both, "timestamp") == T.RecordLayout(24, 8, 12, 16, 0, T.T_F64)
    assert T.layout_of(both, False).t_type == T.T_NONE
    for lay in R.LAYOUTS.values():                                                        # the test layouts are the helper's
        assert T.layout_of(R.view_dtype(lay), "t" if lay.t_type else False)[:4] == lay[:4]
    bad = [np.dtype([("x", ">f4"), ("y", "<f4"), ("z", "<f4")]),                           # big-endian coordinate
           np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8")]),                           # float64 coordinates
           np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<i4")]),
           np.dtype([("x", "<f4"), ("y", "<f4")] + [("pad", "u1", (4,))]),                 # no z
           np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<u8")]),             # unsupported time dtypes
           np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<f2")]),
           np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", ">u4")]),             # big-endian time
           np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<f4", (2,))]),
           np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "u1", (245,))]),    # itemsize 257
           np.dtype(dict(names=["x", "y", "z"], formats=["<f4"] * 3, offsets=[0, 2, 6], itemsize=10)),  # itemsize 10
           np.dtype("<f4")]
    for dt in bad:
        with pytest.raises(ValueError):
            T.layout_of(dt)
    with pytest.raises(ValueError):
        T.layout_of(np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]), "time")          # a named field that is not there
    arr = np.zeros(5, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("t", "<u4")]))
    assert T.resolve(arr) == (5, T.RecordLayout(16, 0, 4, 8, 12, T.T_U32))
    raw = arr.view(np.uint8).reshape(5, 16)
    assert T.resolve(raw, layout=(16, 0, 4, 8, 12, 6)) == T.resolve(arr)
    for args in [(raw,), (arr[::2],), (raw, None, (15, 0, 4, 8, 0, 0)), (raw.astype(np.int8), None, (16, 0, 4, 8, 0, 0)),
                 (raw, None, (16, 0, 4, 13, 0, 0)), (raw, None, (16, 0, 4, 8, 12, 3)), ([1, 2, 3],)]:
        with pytest.raises(ValueError):
            T.resolve(*args)
