"""The host twins of the per-point attribute (madicp_host_ingest_sources_attr, madicp_host_cloud_export_f32_attr,
madicp_host_map_*_attr: include/madicp_host.h) against the numpy restatement of tests/attribute_ref.py, word for word, and the
Python side's attribute_of.  No GPU: the device calls are held to the same restatement in tests/test_gpu_attribute.py."""
import ctypes as C

import numpy as np
import pytest

import attribute_ref as A
import cloud_export_ref as E
import ingest_sources_ref as S
import voxel_map_ref as V
from mad_icp_amd import capi, records
from mad_icp_amd.records import T_F32, T_NONE, T_U32, RecordLayout

pytestmark = pytest.mark.usefixtures("natives")


def check_ingest(sources, t_range=None):
    want = A.ingest(sources, t_range)
    got = capi.host_ingest_sources_attr(sources, t_range)
    plain = capi.host_ingest_sources([_without(s) for s in sources], t_range)
    assert S.R.same_bits(got[0], want[0]) and got[3] == want[3]
    assert got[4].dtype == np.uint32 and np.array_equal(got[4], want[4])
    # points and stamps are those of the call without the attribute
    assert got[0].tobytes() == plain[0].tobytes() and got[2:4] == plain[2:4]
    assert (got[1] is None) == (plain[1] is None) and (got[1] is None or got[1].tobytes() == plain[1].tobytes())
    return got


def _without(src):
    import copy

    s = copy.copy(src)
    s.attribute = None
    return s


@pytest.mark.parametrize("code", A.CODES)
def test_every_type_over_the_eight_layouts(code):
    sources, t_range = S.case_e()
    check_ingest(A.with_attribute(sources, code), t_range)


@pytest.mark.parametrize("code", A.CODES)
@pytest.mark.parametrize("step", [13, 22, 26, 256])
def test_field_in_the_last_bytes_of_the_record(step, code):
    lay = RecordLayout(step, 0, 4, 8, 0, T_NONE) if step == 13 else RecordLayout(step, 0, 4, 8, 12, T_F32)
    src = A.with_attribute([S.source(lay, 301, 40 + step)], code, last_bytes=True)
    assert src[0].attribute[0] + A.WIDTH[code] == step
    check_ingest(src)


@pytest.mark.parametrize("off", [1, 2, 3, 5, 6, 7, 13, 15])
def test_offsets_that_straddle_a_dword(off):
    for code in (3, 4, 5, 6, 7):
        src = S.source(RecordLayout(22, 0, 4, 8, 18, T_U32), 257, 50 + off)
        src.attribute = (off, code)
        check_ingest([src])


def test_one_record_and_the_word_itself():
    """n = 1; an INT16 of -1 is the word 0x0000ffff and comes back as -1; a float32 keeps its bits, NaN payload and -0.0 included"""
    dt = np.dtype({"names": ["x", "y", "z", "ring", "intensity"], "formats": ["<f4", "<f4", "<f4", "<i2", "<f4"], "offsets": [0, 4, 8, 13, 17],
                   "itemsize": 22})
    rec = np.zeros(3, dt)
    rec["x"], rec["ring"] = 5.0, [-1, 2, -32768]
    rec["intensity"] = np.array([0x7fc12345, 0x80000000, 0x3f800000], "<u4").view("<f4")
    for name, want in (("ring", [0x0000ffff, 2, 0x00008000]), ("intensity", [0x7fc12345, 0x80000000, 0x3f800000])):
        for n in (1, 3):
            src = records.Source(rec[:n], 1.0, 100.0, attribute=name)
            got = capi.host_ingest_sources_attr([src])
            assert got[0].shape == (n, 3) and got[4].tolist() == want[:n]
            off, code, fdt = records.attribute_of(dt, name)
            back = records.attribute_view(got[4], fdt)
            assert back.dtype == fdt and back.tobytes() == np.ascontiguousarray(rec[name][:n]).tobytes()
            assert np.array_equal(got[4], A.words(rec[:n], off, code))


def _call(sources, fields, out_attr=True):
    alive, arr, total, _, tr = capi._sources_args(sources, None)
    f = None
    if fields is not None:
        f = (capi.AttrFieldC * len(fields))(*[capi.AttrFieldC(o, t) for o, t in fields])
    xyz, st, w = np.full((total, 3), 7.0), np.full(total, 7.0), np.full(total, 0xdeadbeef, np.uint32)
    kept = C.c_int64(-5)
    rc = capi.host_lib().madicp_host_ingest_sources_attr(arr, len(sources), f, None, xyz.ctypes.data_as(capi._dp), st.ctypes.data_as(capi._dp),
                                                         w.ctypes.data_as(capi._u32p) if out_attr else None, C.byref(kept), None, None)
    untouched = kept.value == -5 and (xyz == 7.0).all() and (st == 7.0).all() and (w == 0xdeadbeef).all()
    return rc, untouched


def test_refusals_write_nothing():
    a, b = S.source(S.L22, 300, 60), S.source(S.L16, 200, 61)
    bad = [("type 0 beside a field", [(3, 7), (0, 0)]), ("a field beside type 0", [(0, 0), (3, 7)]), ("differing types", [(3, 7), (3, 6)]),
           ("unknown type 8", [(3, 8), (3, 8)]), ("negative type", [(3, -1), (3, -1)]), ("negative offset", [(-1, 2), (0, 2)]),
           ("float32 past the end of 22", [(19, 7), (3, 7)]), ("float32 past the end of 16", [(3, 7), (13, 7)]),
           ("int16 past the end", [(21, 3), (3, 3)]), ("uint8 past the end", [(22, 2), (3, 2)])]
    for why, fields in bad:
        rc, untouched = _call([a, b], fields)
        assert rc == -1 and untouched, why
    rc, untouched = _call([a, b], [(18, 7), (12, 7)], out_attr=False)  # (legal fields, nowhere to put the words)
    assert rc == -1 and untouched
    # the legal neighbours of the offsets above
    assert _call([a, b], [(18, 7), (12, 7)])[0] == 0 and _call([a, b], [(20, 3), (14, 3)])[0] == 0 and _call([a, b], [(21, 2), (15, 2)])[0] == 0
    # no fields: madicp_host_ingest_sources, out_attr not written and not needed
    assert _call([a, b], None, out_attr=False)[0] == 0


def test_attribute_of_errors():
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("i", "<f4"), ("big", ">u2"), ("wide", "<f8"), ("long", "<i8"), ("vec", "<u1", (2,)),
                   ("ring", "<u1")])
    assert records.attribute_of(dt, "i") == (12, records.A_FLOAT32, np.dtype("<f4"))
    assert records.attribute_of(dt, "ring") == (dt.fields["ring"][1], records.A_UINT8, np.dtype("u1"))
    for code, fdt in records.ATTR_DTYPE.items():
        assert records.attribute_of(np.dtype([("a", fdt)]), "a") == (0, code, fdt)
    for name in ("missing", "big", "wide", "long", "vec"):
        with pytest.raises(ValueError):
            records.attribute_of(dt, name)
    with pytest.raises(ValueError):
        records.attribute_of(np.dtype("<f4"), "x")
    with pytest.raises(ValueError):
        records.resolve_attribute(np.zeros((2, 16), np.uint8), (3, 9))
    with pytest.raises(ValueError):
        records.resolve_attribute(np.zeros((2, 16), np.uint8), "x")
    assert records.resolve_attribute(np.zeros((2, 16), np.uint8), (3, 4)) == (3, records.A_UINT16, np.dtype("<u2"))


def test_resolve_sources_errors():
    """what Pipeline.computeSourcesStamped refuses before it calls the native layers"""
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("i", "<f4"), ("ring", "<u2"), ("big", ">f4")])
    a, b = np.zeros(3, dt), np.zeros(4, dt)
    ok = records.resolve_sources([records.Source(a, 1.0, 9.0, attribute="i"), records.Source(b, 1.0, 9.0, attribute=(12, records.A_FLOAT32))])
    assert [r.attribute for r in ok] == [(12, records.A_FLOAT32)] * 2
    assert [r.attribute for r in records.resolve_sources([records.Source(a, 1.0, 9.0)])] == [(0, records.A_NONE)]
    for bad in ([records.Source(a, 1.0, 9.0, attribute="i"), records.Source(b, 1.0, 9.0)],
                [records.Source(a, 1.0, 9.0), records.Source(b, 1.0, 9.0, attribute="i")],
                [records.Source(a, 1.0, 9.0, attribute="i"), records.Source(b, 1.0, 9.0, attribute="ring")],
                [records.Source(a, 1.0, 9.0, attribute="missing")], [records.Source(a, 1.0, 9.0, attribute="big")],
                [records.Source(a, 1.0, 9.0, attribute=(12, 9))], [records.Source(a, 1.0, 9.0, attribute=12)]):
        with pytest.raises(ValueError):
            records.resolve_sources(bad)


@pytest.mark.parametrize("n", [1, 64, 65, 1025, 4097])
def test_export_twin(n):
    attr = A.hashed(n, n)
    for name, pts in E.input_sets(n, 200 + n):
        for voxel in (0.0, 0.5, 1e6):
            R, t = E.IDENTITY if name in ("one_cell", "own_cells", "two_cells") else E.random_pose(n)
            rows, w = capi.host_cloud_export_f32_attr(pts, attr, R, t, voxel)
            want_rows, want_w = A.export(pts, attr, R, t, voxel)
            assert E.same_bits(rows, want_rows) and np.array_equal(w, want_w), (name, voxel)
            assert rows.tobytes() == capi.host_cloud_export_f32(pts, R, t, voxel).tobytes()
            if name == "one_cell" and voxel > 0:
                assert w.tolist() == [int(attr[0])]


def test_export_refusals():
    pts, attr = E.gaussian(10, 1), A.hashed(10)
    R, t = E.IDENTITY
    L = capi.host_lib()
    out, ow, m = np.full((10, 3), 7.0, np.float32), np.full(10, 0xdeadbeef, np.uint32), C.c_int64(-5)
    fp = C.POINTER(C.c_float)
    args = lambda a, o, cap: (pts.ctypes.data_as(capi._dp), a, 10, np.ascontiguousarray(R).ctypes.data_as(capi._dp),  # noqa: E731
                              np.ascontiguousarray(t).ctypes.data_as(capi._dp), 0.0, out.ctypes.data_as(fp), o, cap, C.byref(m))
    assert L.madicp_host_cloud_export_f32_attr(*args(None, ow.ctypes.data_as(capi._u32p), 10)) == -1
    assert L.madicp_host_cloud_export_f32_attr(*args(attr.ctypes.data_as(capi._u32p), None, 10)) == -1
    assert m.value == -5
    assert L.madicp_host_cloud_export_f32_attr(*args(attr.ctypes.data_as(capi._u32p), ow.ctypes.data_as(capi._u32p), 9)) == -4
    assert m.value == 10 and (out == 7.0).all() and (ow == 0xdeadbeef).all()


@pytest.mark.parametrize("n", [1, 65, 1025])
def test_map_twin(n):
    ref, h, plain = A.AttrMap(V.VOXEL), capi.host_map_create_attr(V.VOXEL, 1, 1 << 24), capi.host_map_create(V.VOXEL, 1, 1 << 24)
    try:
        prev = 0
        for f, (pts, R, t, added, want) in enumerate(V.reference(n, "random")):
            attr = None if f == 1 else A.hashed(n, 1000 * f)  # (frame 1: a cloud without a column contributes zeros)
            assert ref.insert(pts, attr, R, t) == added
            assert capi.host_map_insert_attr(h, pts, attr, R, t) == (added, want.shape[0]) == capi.host_map_insert(plain, pts, R, t)
            for first in (0, prev):
                rows = capi.host_map_download_f32(h, first)
                assert E.same_bits(rows, want[first:]) and rows.tobytes() == capi.host_map_download_f32(plain, first).tobytes()
                assert np.array_equal(capi.host_map_download_attr(h, first), ref.attr(first))
            prev = want.shape[0]
        with pytest.raises(capi.MadIcpError):
            capi.host_map_download_attr(plain)
        capi.host_map_clear(h)
        assert capi.host_map_size(h) == 0 and capi.host_map_download_attr(h).shape == (0,)
    finally:
        capi.host_map_destroy(h)
        capi.host_map_destroy(plain)


def test_map_first_word_stays():
    R, t = E.IDENTITY
    h = capi.host_map_create_attr(0.5, 1, 100)
    try:
        pts = E.one_cell(5, 1)
        assert capi.host_map_insert_attr(h, pts, [11, 12, 13, 14, 15], R, t) == (1, 1)
        assert capi.host_map_insert_attr(h, pts, [21, 22, 23, 24, 25], R, t) == (0, 1)
        assert capi.host_map_download_attr(h).tolist() == [11]
    finally:
        capi.host_map_destroy(h)
