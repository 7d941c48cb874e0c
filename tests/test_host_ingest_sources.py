"""The host twin of the multi-source ingest (madicp_host_ingest_sources, csrc/host/ingest_records.h) against the numpy restatement
of tests/ingest_sources_ref.py, bit for bit over the case table, and every refusal with nothing written.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ingest_records_ref as R
import ingest_sources_ref as SR
from mad_icp_amd import capi, synth


def check(sources, t_range=None):
    ref_p, ref_s, ref_r, ref_per = SR.reference(sources, t_range)
    pts, st, rng, per = capi.host_ingest_sources(sources, t_range)
    assert per == ref_per and pts.shape[0] == sum(per)
    assert R.same_bits(pts, ref_p)
    assert R.same_bits(np.array(rng), np.array(ref_r)), (rng, ref_r)
    if ref_s is None:
        assert st is None
    else:
        assert R.same_bits(st, ref_s)
    return pts, st, rng, per


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_case_table(natives, name):
    sources, t_range = SR.CASES[name]()
    pts, st, rng, per = check(sources, t_range)
    if name == "A":  # one plain source IS the single-source ingest
        s = sources[0]
        p1, s1, r1 = capi.host_ingest_records(s.records, s.min_range, s.max_range, 0, layout=s.layout)
        assert R.same_bits(pts, p1) and R.same_bits(st, s1) and R.same_bits(np.array(rng), np.array(r1))
    if name == "C":
        assert per == [1, 1, 1]
    if name == "D":
        assert st is None and rng == (np.inf, -np.inf)
    if name == "E":
        assert len(per) == 8 and all(0 < k for k in per) and np.nanmin(st) == 0.0 and np.nanmax(st) == 1.0
    if name == "F":
        assert per[0] == 0 and per[1] > 0 and rng[0] == 0.0 and st.min() > 0.0  # the minimum sits in a dropped record
    if name == "G":
        assert per == [0, 0] and pts.shape == (0, 3)
    if name == "H":
        assert np.isnan(st).all() and rng == (5.0, 5.0)
    if name == "I":
        assert rng == t_range and st.min() < 0.0 and st.max() > 1.0
    if name == "M":
        assert per[0] > 200000 and per[1] > 0


def test_signed_zero_times_of_a_plain_source_stay_as_they_are(natives):
    """t_scale == 1, t_offset == 0 takes the time as it is: with an explicit range below zero a -0.0 time keeps its stamp's bits"""
    n = 64
    t = np.zeros(n, "<f4")
    t[::2] = -0.0
    src = SR.source(SR.L16, n, 40, keep=np.ones(n, bool), times=t)
    pts, st, _, _ = check([src], (-1.0, 1.0))
    p1, s1, _ = capi.host_ingest_records(src.records, src.min_range, src.max_range, 0, layout=src.layout, t_range=(-1.0, 1.0))
    assert R.same_bits(st, s1) and R.same_bits(pts, p1)


def test_exact_reassembly(natives):
    """case L: a scan split into an identity source and a rotated, time-shifted one merges back into the single-source ingest"""
    scan = SR.quantised(synth.render_scan(synth.Scene(0), synth.path_pose(2.0), 7, n_beams=16, n_azimuth=450))
    rng = np.random.default_rng(50)
    far = np.full((40, 3), 400.0, np.float32)
    xyz = np.insert(scan, rng.integers(0, scan.shape[0], size=40), far, axis=0)
    ticks = rng.integers(SR.TIME_SHIFT, 10**8, size=xyz.shape[0]).astype("<u4")
    whole, sources = SR.reassembly(xyz, ticks)
    pts, st, r, per = check(sources)
    p1, s1, r1 = capi.host_ingest_records(whole, SR.LO, SR.HI, 0, layout=SR.L22)
    assert pts.shape == p1.shape == (scan.shape[0], 3) and sum(per) == scan.shape[0]
    assert np.array_equal(pts, p1) and np.array_equal(st, s1) and r == r1
    assert np.array_equal(pts, scan.astype(np.float64))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _raw_call(sources, t_range=None, null=()):
    """madicp_host_ingest_sources with sentinel-filled outputs; returns (rc, outputs untouched)"""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    _alive, arr, count, tr = SR.native_args(sources, t_range)
    xyz, st, rng = np.full((4096, 3), -7.0), np.full(4096, -7.0), np.full(2, -7.0)
    kept, per = C.c_int64(-7), np.full(16, -7, np.int64)
    rc = capi.host_lib().madicp_host_ingest_sources(
        None if "sources" in null else arr, count, None if tr is None else tr.ctypes.data_as(dp),
        None if "xyz" in null else xyz.ctypes.data_as(dp), st.ctypes.data_as(dp), None if "n" in null else C.byref(kept),
        per.ctypes.data_as(ip), rng.ctypes.data_as(dp))
    untouched = (xyz == -7.0).all() and (st == -7.0).all() and (rng == -7.0).all() and kept.value == -7 and (per == -7).all()
    return rc, bool(untouched)


BAD = SR.bad_source_sets()


@pytest.mark.parametrize("why,sources,t_range", BAD, ids=[b[0] for b in BAD])
def test_refusals_write_nothing(natives, why, sources, t_range):
    rc, untouched = _raw_call(sources, t_range)
    assert rc == -1 and untouched, why


def test_null_arguments(natives):
    s = [SR.source(SR.L22, 300, 60)]
    for null in ("sources", "xyz", "n"):
        rc, untouched = _raw_call(s, null=(null,))
        assert rc == -1 and untouched, null
    _alive, arr, _, _ = SR.native_args(s, None)
    arr[0].data = None
    xyz, kept = np.full((300, 3), -7.0), C.c_int64(-7)
    L = capi.host_lib()
    assert L.madicp_host_ingest_sources(arr, 1, None, xyz.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(kept), None, None) == -1
    assert kept.value == -7 and (xyz == -7.0).all()
    rc, untouched = _raw_call(s)                                      # ... and the same call with nothing wrong is taken
    assert rc == 0 and not untouched


def test_optional_outputs_may_be_null(natives):
    sources, _ = SR.CASES["B"]()
    ref_p, _, _, _ = SR.reference(sources)
    _alive, arr, total, _, _ = capi._sources_args(sources, None)
    xyz, kept = np.empty((total, 3)), C.c_int64(0)
    rc = capi.host_lib().madicp_host_ingest_sources(arr, 2, None, xyz.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(kept), None, None)
    assert rc == 0 and R.same_bits(xyz[:kept.value], ref_p)
