"""The host twin of the voxel map (madicp_host_map_*, csrc/host/voxel_map.h) against the numpy restatement of
tests/voxel_map_ref.py, bit for bit (cloud_export_ref.same_bits) after every fold, and every refusal with the map unchanged.
No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloud_export_ref as E
import voxel_map_ref as V
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)

INVALID, CAPACITY = -1, -4
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)


@pytest.fixture
def new_map(maps):
    return functools.partial(maps.host, max_rows=1 << 30)


@pytest.mark.parametrize("kind", ["identity", "random"])
@pytest.mark.parametrize("n", V.SIZES)
def test_sequences_bit_for_bit(new_map, n, kind):
    m = new_map(V.VOXEL)
    seq = V.reference(n, kind)
    assert 3 <= len(seq) <= 6
    prev = np.empty((0, 3), np.float32)
    for pts, R, t, added, want in seq:
        got_added, got_rows = m.insert(pts, R, t)
        assert (got_added, got_rows) == (added, want.shape[0]) and m.size() == want.shape[0]
        got = m.rows()
        assert got.dtype == np.float32 and E.same_bits(got, want)
        assert got[:prev.shape[0]].tobytes() == prev.tobytes()  # prefix stability: a fold changes no row
        assert E.same_bits(m.rows(prev.shape[0]), want[prev.shape[0]:])  # the window of what this fold added
        prev = got
    assert prev.shape[0] > 0


def test_same_cloud_twice_one_cell_own_cells(new_map):
    R, t = E.IDENTITY
    m = new_map(V.VOXEL)
    pts = E.gaussian(3000, 5)
    first, _ = m.insert(pts, R, t)
    assert 100 < first < 3000
    assert m.insert(pts, R, t) == (0, first)  # the same cloud again: nothing is new
    Rr, tr = E.random_pose(2)
    again, rows = m.insert(pts, Rr, tr)  # ... at another pose some of it is
    assert 0 < again < 3000 and rows == first + again
    m = new_map(V.VOXEL)
    assert [m.insert(E.one_cell(500, s), R, t)[0] for s in (1, 2, 3)] == [1, 0, 0]
    assert E.same_bits(m.rows(), E.one_cell(500, 1)[:1].astype(np.float32))  # ... and it is frame 0's row 0
    n = 777
    m = new_map(V.VOXEL, initial_rows=1, max_rows=n)
    assert m.insert(E.own_cells(n), R, t) == (n, n)  # fits exactly
    assert E.same_bits(m.rows(), E.own_cells(n).astype(np.float32))
    m2 = new_map(V.VOXEL, initial_rows=1, max_rows=n - 1)
    a = C.c_int64(-7)
    assert _insert(m2, E.own_cells(n), 1.0 * np.eye(3).reshape(9), np.zeros(3), a, a) == CAPACITY and a.value == -7 and m2.size() == 0


def test_initial_rows_does_not_show(new_map):
    small, large = new_map(V.VOXEL, initial_rows=1), new_map(V.VOXEL, initial_rows=1 << 20)
    for pts, R, t, added, want in V.reference(4097, "random"):
        assert small.insert(pts, R, t) == large.insert(pts, R, t) == (added, want.shape[0])
    assert small.rows().tobytes() == large.rows().tobytes() and small.size() > 4097


def test_download_windows_concatenate(new_map):
    m = new_map(V.VOXEL)
    seq = V.reference(1025, "random")
    sizes = [0]
    windows = []
    for pts, R, t, _, _ in seq:
        m.insert(pts, R, t)
        windows.append(m.rows(sizes[-1]))
        sizes.append(m.size())
    whole = m.rows()
    assert np.concatenate(windows, axis=0).tobytes() == whole.tobytes() and E.same_bits(whole, seq[-1][4])
    assert m.rows(sizes[-1]).shape == (0, 3)
    mid = sizes[-1] // 2
    assert m.rows(mid).tobytes() == whole[mid:].tobytes()


def test_clear_then_the_same_sequence(new_map):
    m = new_map(V.VOXEL)
    seq = V.reference(257, "random")
    for pts, R, t, _, _ in seq:
        m.insert(pts, R, t)
    first = m.rows()
    m.clear()
    assert m.size() == 0 and m.rows().shape == (0, 3)
    for pts, R, t, added, want in seq:
        assert m.insert(pts, R, t) == (added, want.shape[0])
    assert m.rows().tobytes() == first.tobytes()


@pytest.mark.parametrize("voxel", [1e-3, 0.5, 50.0, 1e6])
def test_range_edge(new_map, voxel):
    R, t = E.IDENTITY
    m, ref = new_map(voxel), V.RefMap(voxel)
    pts = E.range_edge(voxel)
    assert m.insert(pts, R, t)[0] == ref.insert(pts, R, t) == 5
    assert E.same_bits(m.rows(), pts[[1, 3, 5, 6, 8]].astype(np.float32)) and E.same_bits(m.rows(), ref.rows())


def test_nonfinite_and_empty(new_map):
    R, t = E.IDENTITY
    m = new_map(V.VOXEL)
    pts = np.array([[1.0, 2.0, 3.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [4.0, 5.0, 6.0], [1e30, 0.0, 0.0]])
    assert m.insert(pts, R, t) == (2, 2) and m.rows().tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    assert m.insert(pts[1:4], R, t) == (0, 2)  # no candidate at all
    assert m.insert(np.empty((0, 3)), R, t) == (0, 2)  # an empty cloud
    a, r = C.c_int64(-7), C.c_int64(-7)
    assert capi.host_lib().madicp_host_map_insert(m.h, None, 0, np.eye(3).ctypes.data_as(_dp), np.zeros(3).ctypes.data_as(_dp), C.byref(a),
                                                  C.byref(r)) == 0 and (a.value, r.value) == (0, 2)
    ref = V.RefMap(V.VOXEL)
    noisy = E.with_nonfinite(E.gaussian(2000, 3), 4)
    m = new_map(V.VOXEL)
    assert m.insert(noisy, R, t)[0] == ref.insert(noisy, R, t) and E.same_bits(m.rows(), ref.rows()) and np.isfinite(m.rows()).all()


def test_the_key_comes_from_the_fp64_position(new_map):
    """x = nextafter(0.5, 0) is stored as float 0.5 but lies in cell 0 at voxel 0.5; x = 0.5 exactly lies in cell 1: it is new, and
    the map then holds two rows whose floats are equal.  A key taken from the stored float would drop it."""
    R, t = E.IDENTITY
    below = np.array([[np.nextafter(0.5, 0.0), 0.25, 0.25]])
    exact = np.array([[0.5, 0.25, 0.25]])
    assert np.float32(below[0, 0]) == np.float32(0.5) and below[0, 0] < 0.5
    m, ref = new_map(0.5), V.RefMap(0.5)
    assert m.insert(below, R, t) == (1, 1) and ref.insert(below, R, t) == 1
    assert m.insert(exact, R, t) == (1, 2) and ref.insert(exact, R, t) == 1
    assert m.insert(below, R, t) == (0, 2) and ref.insert(below, R, t) == 0
    got = m.rows()
    assert got.tobytes() == ref.rows().tobytes() and got[0].tobytes() == got[1].tobytes() and got[0, 0] == np.float32(0.5)


def _insert(m, pts, R, t, added, rows, n=None):
    return capi.host_lib().madicp_host_map_insert(m.h, None if pts is None else pts.ctypes.data_as(_dp), pts.shape[0] if n is None else n,
                                                  None if R is None else R.ctypes.data_as(_dp), None if t is None else t.ctypes.data_as(_dp),
                                                  None if added is None else C.byref(added), None if rows is None else C.byref(rows))


def test_refusals_leave_the_map_alone(new_map):
    L = capi.host_lib()
    h = C.c_void_p(7)
    for voxel, initial, max_rows in ((0.0, 1, 10), (-0.5, 1, 10), (np.nan, 1, 10), (np.inf, 1, 10), (0.5, 0, 10), (0.5, 1, 0),
                                     (0.5, 1, (1 << 30) + 1)):
        assert L.madicp_host_map_create(voxel, initial, max_rows, C.byref(h)) == INVALID and h.value == 7
    assert L.madicp_host_map_create(0.5, 1, 10, None) == INVALID
    m = new_map(V.VOXEL, initial_rows=4, max_rows=600)
    pts = np.ascontiguousarray(E.gaussian(500, 9))
    R, t = np.eye(3).reshape(9).copy(), np.zeros(3)
    added, rows = m.insert(pts, R, t)
    before = m.rows().tobytes()
    a, r = C.c_int64(-7), C.c_int64(-7)
    assert _insert(m, pts, None, t, a, r) == INVALID
    assert _insert(m, pts, R, None, a, r) == INVALID
    assert _insert(m, pts, R, t, None, r) == INVALID
    assert _insert(m, pts, R, t, a, None) == INVALID
    assert _insert(m, pts, R, t, a, r, n=-1) == INVALID
    assert L.madicp_host_map_insert(m.h, None, 5, R.ctypes.data_as(_dp), t.ctypes.data_as(_dp), C.byref(a), C.byref(r)) == INVALID
    assert L.madicp_host_map_insert(None, pts.ctypes.data_as(_dp), 5, R.ctypes.data_as(_dp), t.ctypes.data_as(_dp), C.byref(a), C.byref(r)) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        Rb, tb = R.copy(), t.copy()
        Rb[4] = bad
        tb[2] = bad
        assert _insert(m, pts, Rb, t, a, r) == INVALID
        assert _insert(m, pts, R, tb, a, r) == INVALID
    # max_rows: rows + n > max_rows is refused before a point is looked at, even where most points would not be new
    assert rows + 500 > 600 and _insert(m, pts, R, t, a, r) == CAPACITY
    assert (a.value, r.value) == (-7, -7) and m.size() == rows and m.rows().tobytes() == before
    assert m.insert(pts[:600 - rows], R, t) == (0, rows)  # what still fits is folded
    # download: too little room — the number needed, nothing written; a first_row beyond the map
    sentinel = np.float32(-77.5)
    out = np.full((rows, 3), sentinel, np.float32)
    k = C.c_int64(-7)
    f = L.madicp_host_map_download_f32
    assert f(m.h, 0, out.ctypes.data_as(_fp), rows - 1, C.byref(k)) == CAPACITY and k.value == rows and (out == sentinel).all()
    k.value = -7
    assert f(m.h, rows + 1, out.ctypes.data_as(_fp), rows, C.byref(k)) == INVALID and f(m.h, -1, out.ctypes.data_as(_fp), rows, C.byref(k)) == INVALID
    assert f(m.h, 0, None, rows, C.byref(k)) == INVALID and f(m.h, 0, out.ctypes.data_as(_fp), rows, None) == INVALID
    assert f(None, 0, out.ctypes.data_as(_fp), rows, C.byref(k)) == INVALID
    assert k.value == -7 and (out == sentinel).all()
    assert f(m.h, 3, out.ctypes.data_as(_fp), rows - 3, C.byref(k)) == 0 and k.value == rows - 3  # exactly enough is enough
    assert out[:rows - 3].tobytes() == before[36:] and (out[rows - 3:] == sentinel).all()
    assert L.madicp_host_map_size(None, C.byref(k)) == INVALID and L.madicp_host_map_size(m.h, None) == INVALID
    assert L.madicp_host_map_clear(None) == INVALID
    L.madicp_host_map_destroy(None)
