"""The host twin's prune (madicp_host_map_prune, csrc/host/voxel_map.h: VoxelMap::prune) against the numpy restatement of
tests/map_prune_ref.py after EVERY step of the shared sequences, bit for bit, with and without the attribute column; every
refusal with the map unchanged.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloud_export_ref as E
import map_prune_ref as P
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)

INVALID = -1
_dp = C.POINTER(C.c_double)


TWIN = dict(voxel=P.VOXEL, with_attr=True)  # what this suite's maps are unless a test says otherwise


@pytest.fixture
def twins(maps):
    return functools.partial(maps.host, **TWIN)


@pytest.mark.parametrize("name", P.SIZE_NAMES)
def test_sizes_and_radii(twins, name):
    want = P.replay(name, twins())
    n, mode = int(name.split("-")[1]), name.split("-")[2]
    (added, rows), (removed, left, mark) = want[0][0], want[1][0]
    assert added == rows == n  # every point a row: the prune sees exactly n rows
    if mode == "none":
        assert (removed, left, mark) == (0, n, n)
    elif mode == "all":
        assert (removed, left, mark) == (n, 0, 0)
    elif mode == "alternate":
        assert (removed, left) == (n // 2, n - n // 2) and want[1][2].tolist() == list(range(0, n, 2))
    else:
        assert n // 2 <= left <= n // 2 + 1  # cut at the median distance (the median row itself may fall on either side)
    # the cloud again: exactly the removed voxels are new, at the end, in index order; the same prune removes exactly those
    assert want[2][0] == (removed, n) and want[3][0][:2] == (removed, left)
    assert want[3][1].tobytes() == want[1][1].tobytes() and want[3][2].tobytes() == want[1][2].tobytes()


@pytest.mark.parametrize("with_attr", [False, True])
@pytest.mark.parametrize("name", P.OTHER_NAMES + ["large"])
def test_sequences(twins, name, with_attr):
    P.replay(name, twins(initial_rows=1, with_attr=with_attr))


def test_boundary_rows(twins):
    want = P.replay("boundary", twins())
    ans, rows, words = want[1]
    assert ans == (3, 3, 2) and words.tolist() == [0, 1, 4]
    assert rows.tolist() == [[3.0, 4.0, 0.0], [0.0, 0.0, 5.0], [-5.0, 0.0, 0.0]]


def test_watermarks(twins):
    steps, want = P.expected("reentry")
    keep = P.RefPruneMap(P.VOXEL)
    keep.insert(steps[0][1], steps[0][2], steps[0][3])
    mask = keep.kept_mask(steps[1][1], steps[1][2])
    n = mask.shape[0]
    for wm in (0, 1, n // 2, n - 1, n):
        m = twins()
        m.insert(steps[0][1], steps[0][2], steps[0][3], None)
        assert m.prune(steps[1][1], steps[1][2], wm) == (n - int(mask.sum()), int(mask.sum()), int(mask[:wm].sum()))


def test_reentry_order(twins):
    want = P.replay("reentry", twins())
    n = 1025
    assert want[1][2].tolist() == list(range(0, n, 2))  # the inner shell stays
    assert want[2][0] == (n // 2, n) and want[2][2].tolist() == list(range(0, n, 2)) + list(range(1, n, 2))  # ... the outer one returns
    assert want[3][0] == (n // 2, n - n // 2, n // 2)  # (watermark n // 2: all of rows [0, n // 2) are inner ones)
    assert want[3][2].tolist() == list(range(0, n, 2))


def test_prune_to_empty_then_a_fold_is_a_first_fold(twins):
    want = P.replay("to_empty", twins())
    assert want[1][0][1] == 0 and want[2][0] == want[0][0] and want[2][1].tobytes() == want[0][1].tobytes()


def test_a_prune_that_removes_nothing_does_not_show(twins):
    a, b = twins(), twins()
    for f in range(3):
        pts = E.gaussian(1025, 40 + f)
        R, t = E.random_pose(f)
        words = np.arange(1025, dtype=np.uint32)
        assert a.insert(pts, R, t, words) == b.insert(pts, R, t, words)
        assert a.prune(np.zeros(3), 1.0e5, 7)[0::2] == (0, 7)
        assert a.rows().tobytes() == b.rows().tobytes() and a.words().tobytes() == b.words().tobytes()


def test_the_key_is_the_stored_one(twins):
    """two rows whose floats are equal but whose fp64 positions lie in different cells (test_host_voxel_map): a prune that keeps
    both must keep both KEYS — keys recomputed from the floats would let `below` in again"""
    R, t = E.IDENTITY
    below, exact = np.array([[np.nextafter(0.5, 0.0), 0.25, 0.25]]), np.array([[0.5, 0.25, 0.25]])
    far = np.array([[40.0, 0.25, 0.25]])
    m, ref = twins(voxel=0.5), P.RefPruneMap(0.5)
    for pts in (below, exact, far):
        assert m.insert(pts, R, t, None)[0] == ref.insert(pts, R, t) == 1
    assert m.prune(np.zeros(3), 10.0, 3) == ref.prune(np.zeros(3), 10.0, 3) == (1, 2, 2)
    assert m.insert(below, R, t, None) == (0, 2) and m.insert(exact, R, t, None) == (0, 2) and m.insert(far, R, t, None) == (1, 3)


def test_nonfinite_rows_leave(twins):
    """a float row that overflowed to inf on its way out (1e39 is a candidate at voxel 1e34) fails the comparison: removed"""
    R, t = E.IDENTITY
    m, ref = twins(voxel=1e34), P.RefPruneMap(1e34)
    pts = np.array([[1.0, 2.0, 3.0], [1e39, 0.0, 0.0], [0.0, -1e39, 0.0]])
    assert m.insert(pts, R, t, None) == (ref.insert(pts, R, t), 3) and np.isinf(m.rows()).sum() == 2
    assert m.prune(np.zeros(3), 1e150, 3) == ref.prune(np.zeros(3), 1e150, 3) == (2, 1, 1)
    assert m.rows().tolist() == [[1.0, 2.0, 3.0]]


def _prune(h, c, r, wm, a, b, k):
    return capi.host_lib().madicp_host_map_prune(h, None if c is None else c.ctypes.data_as(_dp), r, wm, None if a is None else C.byref(a),
                                                 None if b is None else C.byref(b), None if k is None else C.byref(k))


def test_refusals_leave_the_map_alone(twins):
    m = twins()
    R, t = E.IDENTITY
    rows = m.insert(E.gaussian(500, 9), R, t, np.arange(500, dtype=np.uint32))[1]
    before, before_w = m.rows().tobytes(), m.words().tobytes()
    c = np.zeros(3)
    a, b, k = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    assert _prune(None, c, 1.0, 0, a, b, k) == INVALID
    assert _prune(m.h, None, 1.0, 0, a, b, k) == INVALID
    assert _prune(m.h, c, 1.0, 0, None, b, k) == INVALID and _prune(m.h, c, 1.0, 0, a, None, k) == INVALID
    assert _prune(m.h, c, 1.0, 0, a, b, None) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        cb = c.copy()
        cb[1] = bad
        assert _prune(m.h, cb, 1.0, 0, a, b, k) == INVALID
        assert _prune(m.h, c, bad, 0, a, b, k) == INVALID
    for r in (0.0, -1.0, 1e200):  # (1e200: finite, its square is not)
        assert _prune(m.h, c, r, 0, a, b, k) == INVALID
    assert _prune(m.h, c, 1.0, -1, a, b, k) == INVALID and _prune(m.h, c, 1.0, rows + 1, a, b, k) == INVALID
    assert (a.value, b.value, k.value) == (-7, -7, -7) and m.rows().tobytes() == before and m.words().tobytes() == before_w
    assert _prune(m.h, c, 1e150, rows, a, b, k) == 0 and (a.value, b.value, k.value) == (0, rows, rows)  # (1e150 squared is finite)
    empty = twins()
    assert empty.prune(c, 1.0, 0) == (0, 0, 0)
    assert _prune(empty.h, c, 1.0, 1, a, b, k) == INVALID
