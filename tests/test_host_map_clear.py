"""The host twin's free-space clearing (madicp_host_map_clear_rays, csrc/host/voxel_map.h: VoxelMap::clearRays) against the numpy
restatement of tests/map_clear_ref.py after EVERY step of the shared sequences, bit for bit, with and without the attribute
column — on the input sets of tests/test_host_map_prune.py as well — and every refusal with the map unchanged.  The cases whose
outcome can be worked out by hand are spelled out here, so that the restatement itself is held to something.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloud_export_ref as E
import map_clear_ref as Cl
import map_prune_ref as P
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)

INVALID = -1
_dp = C.POINTER(C.c_double)


TWIN = dict(voxel=Cl.VOXEL, with_attr=True)  # what this suite's maps are unless a test says otherwise


@pytest.fixture
def twins(maps):
    return functools.partial(maps.host, **TWIN)


@pytest.mark.parametrize("name", Cl.SIZE_NAMES)
def test_ray_counts_and_map_sizes(twins, name):
    want = Cl.replay(name, twins())
    m = int(name.split("-")[1])
    (added, rows), (removed, left, _) = want[0][0], want[1][0]
    assert added == rows == m and removed + left == m  # every point a row: the clearing sees exactly m rows
    assert want[2][0] == (removed, m)  # the cloud again: exactly the cleared voxels are new
    assert want[3][0][0] <= removed  # the same rays, stopping a margin short: never more


@pytest.mark.parametrize("with_attr", [False, True])
@pytest.mark.parametrize("name", Cl.OTHER_NAMES + ["large"])
def test_sequences(twins, name, with_attr):
    Cl.replay(name, twins(initial_rows=1, with_attr=with_attr))


def _cells(rows, axis):
    return sorted(int(np.floor(r[axis] / 0.5)) for r in rows.tolist() if all(0.0 < r[a] < 0.5 for a in range(3) if a != axis) and not 0.0 < r[axis] < 0.5)


def test_exact_lengths_by_hand(twins):
    want = Cl.replay("exact_lengths", twins())
    first, under, exact = want[1], want[3], want[5]
    # L == voxel + margin walks ONE sample: cell 1 of the x line leaves (the end point sits in cell 2); one ulp less walks none
    assert first[0] == (5, 13, 13) and _cells(first[1], 0) == [2, 3] and _cells(first[1], 1) == [-3, -2, -1]
    # L - margin == 4 voxels exactly walks FOUR samples: cells 1 .. 4 of the +z line leave (the end point sits in cell 5)
    assert [c for c in _cells(first[1], 2) if c > 0] == [5, 6]
    # one ulp below: three samples — cell -4 stays although no end point protects it; exactly 4 voxels again: it leaves
    assert under[0] == (3, 15, 0) and [c for c in _cells(under[1], 2) if c < 0] == [-6, -5, -4]
    assert exact[0] == (4, 14, 0) and [c for c in _cells(exact[1], 2) if c < 0] == [-6, -5]


def test_edges_by_hand(twins):
    want = Cl.replay("edges", twins())
    ans, rows, _ = want[1]
    x, y = _cells(rows, 0), _cells(rows, 1)
    # the ray with its end outside the key range walks 4096 samples along +x: cells 1 .. 4096 leave, 4097 (x = 2048.75) and 6000 stay;
    # the voxel of the origin (cell 0: not listed by _cells) is protected by the ray of length 0
    assert ans[0] == 13 and [c for c in x if c < 100000] == [4097, 6000] and rows[0].tolist() == [0.25, 0.25, 0.25]
    # +y: the ray one ulp short of voxel + margin walks nothing; -y: two samples, the second in cell -2; the end point in -3
    assert [c for c in y if c < 100000] == [-6, -5, -4, -3, 1, 2, 3, 4, 5]
    # NaN and infinite points walked nothing and protected nothing; the row inside the range's corner is still there ...
    assert rows[-1].tolist() == [524188.25, 524188.25, 0.25]
    # ... until the ray from an origin OUTSIDE the key range to an end outside it passes through: skipped samples, then the walk
    assert want[3][0] == (1, 25, 0) and not (want[3][1] == np.float32(524188.25)).any() and want[4][0] == (1, 26)


def test_protected_by_hand(twins):
    want = Cl.replay("protected", twins())
    # x line: the long ray (ends in cell 8) clears cells 1 .. 7 except cell 4, where the short ray ENDS; y line: the ray's last sample
    # (margin 0) falls into the voxel it ends in, cell 5: it stays, cells 1 .. 4 leave
    assert want[1][0] == (10, 3, 1) and want[1][1].tolist() == [[2.25, 0.25, 0.25], [4.25, 0.25, 0.25], [0.25, 2.75, 0.25]]
    assert want[2][0] == (10, 13)


def test_contended_nothing_everything(twins):
    assert Cl.replay("contended", twins())[1][0] == (1, 300, 0)  # 4 097 rays through one voxel: that row leaves, once
    nothing = Cl.replay("nothing", twins())
    assert nothing[1][0] == (0, 1024, 512) and nothing[1][1].tobytes() == nothing[0][1].tobytes()
    but = Cl.replay("but_the_endpoints", twins())
    assert but[2][0] == (1025, 1025, 0) and but[2][1].tobytes() == but[1][1][1025:].tobytes() and but[3][0] == (1025, 2050)
    every = Cl.replay("everything", twins(initial_rows=1))
    assert every[1][0] == (1025, 0, 0) and every[2][0] == every[0][0] and every[2][1].tobytes() == every[0][1].tobytes()
    assert every[3][0][0] > 4000  # ... and a growth behind it


def test_the_scene(twins):
    """fold, fold, clear: no row is left inside the box, every wall row of frame 1 is still there — frame 2's own end points
    protect the wall"""
    steps, hits_box, frame1, wall = Cl.scene()
    want = Cl.replay("scene", twins())
    rows = want[2][1]
    in_box = (np.abs(rows[:, 0] - 6.0) < 0.25) & (np.abs(rows[:, 1]) < 1.0) & (np.abs(rows[:, 2]) < 0.6)
    assert hits_box.sum() > 100 and want[2][0][0] > 0 and not in_box.any()
    assert not (rows[:, 0] < 9.0).any()  # nothing in front of the wall at all
    first = Cl.RefClearMap(Cl.VOXEL)
    first.insert(frame1, *E.IDENTITY)
    wall_rows = first.rows()[first.rows()[:, 0] > 9.0]
    have = set(map(bytes, rows.view(np.uint8).reshape(-1, 12)))
    assert wall_rows.shape[0] > 50 and all(bytes(r) in have for r in wall_rows.view(np.uint8).reshape(-1, 12))


def test_watermarks(twins):
    steps, _ = Cl.expected("size-1025-257")
    keep = Cl.RefClearMap(Cl.VOXEL)
    keep.insert(steps[0][1], steps[0][2], steps[0][3])
    gone = keep.cleared_mask(*steps[1][1:6])
    n = gone.shape[0]
    assert 0 < gone.sum() < n
    for wm in (0, 1, n // 2, n - 1, n):
        m = twins()
        m.insert(steps[0][1], steps[0][2], steps[0][3], None)
        assert m.clear_rays(*steps[1][1:6], wm) == (int(gone.sum()), n - int(gone.sum()), int((~gone[:wm]).sum()))


@pytest.mark.parametrize("name", ["reentry", "posed", "growth", "size-1025-median"])
def test_on_the_prune_tests_input_sets(twins, name):
    """the folds of tests/test_host_map_prune.py's sequences, every prune followed by a clearing with the cloud folded last, seen
    from the prune's centre: twin against restatement after every step"""
    m, ref = twins(initial_rows=1), Cl.RefClearMap(P.VOXEL)
    last, removed = None, 0
    for step in P.named(name):
        if step[0] == "fold":
            words = np.arange(step[1].shape[0], dtype=np.uint32)
            assert m.insert(step[1], step[2], step[3], words) == (ref.insert(step[1], step[2], step[3], words), ref.size)
            last = step
        else:
            wm = ref.size if step[3] == "all" else int(step[3] * ref.size) if isinstance(step[3], float) else step[3]
            assert m.prune(step[1], step[2], wm) == ref.prune(step[1], step[2], wm)
            origin = (np.asarray(step[1]) - last[3]) @ last[2] + 0.125  # (about the prune's centre, in the cloud's frame)
            wm = ref.size // 3
            got = m.clear_rays(last[1] * 1.25, last[2], last[3], origin, 0.1, wm)
            assert got == ref.clear_rays(last[1] * 1.25, last[2], last[3], origin, 0.1, wm)
            removed += got[0]
        assert E.same_bits(m.rows(), ref.rows()) and m.words().tobytes() == ref.attr().tobytes()
    assert removed > 0


def test_the_key_is_the_stored_one(twins):
    """two rows whose floats are equal but whose fp64 positions lie in different cells: a ray through the lower cell removes that
    row and leaves its twin — a key recomputed from the float would take the wrong one or both"""
    R, t = E.IDENTITY
    below, exact = np.array([[np.nextafter(0.5, 0.0), 0.25, 0.25]]), np.array([[0.5, 0.25, 0.25]])
    m, ref = twins(), Cl.RefClearMap(0.5)
    for pts in (below, exact):
        assert m.insert(pts, R, t, None)[0] == ref.insert(pts, R, t) == 1
    assert m.rows()[0].tobytes() == m.rows()[1].tobytes()
    ray, o = np.array([[0.25, 0.25, 1.25]]), np.array([0.25, 0.25, -1.25])  # along z through cell (0, 0, 0) only
    assert m.clear_rays(ray, R, t, o, 0.0, 1) == ref.clear_rays(ray, R, t, o, 0.0, 1) == (1, 1, 0)
    assert m.insert(exact, R, t, None) == (0, 1) and m.insert(below, R, t, None) == (1, 2)


def _clear(h, x, n, R, t, o, margin, wm, a, b, k):
    p = lambda v: None if v is None else v.ctypes.data_as(_dp)  # noqa: E731
    r = lambda v: None if v is None else C.byref(v)  # noqa: E731
    return capi.host_lib().madicp_host_map_clear_rays(h, p(x), n, p(R), p(t), p(o), margin, wm, r(a), r(b), r(k))


def test_refusals_leave_the_map_alone(twins):
    m = twins()
    R, t = np.eye(3).reshape(9), np.zeros(3)
    rows = m.insert(E.gaussian(500, 9), R, t, np.arange(500, dtype=np.uint32))[1]
    before, before_w = m.rows().tobytes(), m.words().tobytes()
    x, o = np.ascontiguousarray(E.gaussian(300, 10) * 3.0), np.zeros(3)
    a, b, k = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    ok = (m.h, x, 300, R, t, o, 0.0, 0, a, b, k)
    for i in (0, 1, 3, 4, 5, 8, 9, 10):  # every pointer
        assert _clear(*[None if j == i else v for j, v in enumerate(ok)]) == INVALID
    assert _clear(m.h, x, -1, R, t, o, 0.0, 0, a, b, k) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for which in (3, 4, 5):
            args = list(ok)
            args[which] = args[which].copy()
            args[which][1] = bad
            assert _clear(*args) == INVALID
        assert _clear(m.h, x, 300, R, t, o, bad, 0, a, b, k) == INVALID
    assert _clear(m.h, x, 300, R, t, o, -0.5, 0, a, b, k) == INVALID
    assert _clear(m.h, x, 300, R, t, o, 0.0, -1, a, b, k) == INVALID and _clear(m.h, x, 300, R, t, o, 0.0, rows + 1, a, b, k) == INVALID
    assert (a.value, b.value, k.value) == (-7, -7, -7) and m.rows().tobytes() == before and m.words().tobytes() == before_w
    # an empty cloud (a null pointer is fine then) and an empty map answer without touching anything
    assert _clear(m.h, None, 0, R, t, o, 0.0, rows, a, b, k) == 0 and (a.value, b.value, k.value) == (0, rows, rows)
    assert m.rows().tobytes() == before
    empty = twins()
    assert empty.clear_rays(x, R, t) == (0, 0, 0) and _clear(empty.h, x, 300, R, t, o, 0.0, 1, a, b, k) == INVALID
    assert m.clear_rays(x, R, t, o, 0.0, rows)[0] > 0  # (the arguments the refusals were built around do clear something)
