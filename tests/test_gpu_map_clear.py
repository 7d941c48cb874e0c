"""Context.map_clear_rays (madicp_map_clear_rays: fe::ray_flags / fe::map_clear_mark, then the prune's tail — tile scan, fe::map_compact,
the memset and fe::map_rehash) against BOTH the numpy restatement of tests/map_clear_ref.py and the host twin, bit for bit after EVERY
step of the shared sequences: rows, attribute words, the three answers, and — through the fold behind every clearing — the stored
keys.  Ray counts and map sizes around the wavefront, the workgroup and the 1 024-mark scan tile; the per-ray edges; protection;
the contended flag; nothing, nearly everything and everything removed; cap == rows; growth; watermarks; two maps; a map far larger
than any cloud its context has seen; every refusal; the scene the feature is for."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloud_export_ref as E
import map_clear_ref as Cl
from mad_icp_amd import capi
from map_impls import DevImpl, maps  # noqa: F401 (maps is a fixture)
from test_host_map_clear import TWIN

pytestmark = pytest.mark.gpu

INVALID = -1
_dp = C.POINTER(C.c_double)


@pytest.fixture
def made(ctx, maps):
    """device map / host twin factories"""
    return functools.partial(maps.dev, ctx, **TWIN), functools.partial(maps.host, **TWIN)


@pytest.mark.parametrize("name", Cl.SIZE_NAMES)
def test_ray_counts_and_map_sizes(made, name):
    dev, twin = made
    want = Cl.replay(name, dev(), also=(twin(),))
    assert want[0][0][1] == int(name.split("-")[1]) and want[4][0][0] > 0  # rows == M; the last fold grows the 64-row block


@pytest.mark.parametrize("name", Cl.OTHER_NAMES)
def test_sequences(made, name):
    dev, twin = made
    Cl.replay(name, dev(), also=(twin(),))


@pytest.mark.parametrize("name", ["edges", "size-1025-1025", "everything", "but_the_endpoints"])
def test_initial_rows_1_and_no_column(made, name):
    """a block that has grown from one row, and a map without the attribute column: the same rows"""
    dev, _ = made
    Cl.replay(name, dev(initial_rows=1), also=(dev(initial_rows=1, with_attr=False),))


@pytest.mark.parametrize("m", [1, 256, 1025])
def test_cap_equals_rows(made, m):
    """a block that is exactly full (initial_rows == max_rows == rows): the table is exactly half full, the scratch layout at its
    tightest — at cap 1 the 24 bytes of the table region are flags 8 | marks 8 | one tile sum 4 | total 4"""
    dev, twin = made
    R, t = E.IDENTITY
    cells = E.own_cells(m)
    rays = Cl.through(cells[::2], Cl.ORIGIN, np.full(cells[::2].shape[0], 1.6))
    d, h, ref = dev(initial_rows=m, max_rows=m), twin(initial_rows=m, max_rows=m), Cl.RefClearMap(Cl.VOXEL)
    words = np.arange(m, dtype=np.uint32)
    assert d.insert(cells, R, t, words) == h.insert(cells, R, t, words) == (ref.insert(cells, R, t, words), m)
    want = ref.clear_rays(rays, R, t, Cl.ORIGIN, 0.0, m)
    assert d.clear_rays(rays, R, t, Cl.ORIGIN, 0.0, m) == h.clear_rays(rays, R, t, Cl.ORIGIN, 0.0, m) == want and want[0] > 0
    assert E.same_bits(d.rows(), ref.rows()) and d.words().tobytes() == ref.attr().tobytes() == h.words().tobytes()
    added = ref.insert(cells[:want[0]], R, t, words[:want[0]])  # (as many points as rows left: still within max_rows)
    assert d.insert(cells[:want[0]], R, t, words[:want[0]]) == h.insert(cells[:want[0]], R, t, words[:want[0]]) == (added, ref.size)
    assert E.same_bits(d.rows(), ref.rows()) and d.words().tobytes() == ref.attr().tobytes()


def test_watermarks(made):
    dev, _ = made
    steps, _ = Cl.expected("size-1025-257")
    keep = Cl.RefClearMap(Cl.VOXEL)
    keep.insert(steps[0][1], steps[0][2], steps[0][3])
    gone = keep.cleared_mask(*steps[1][1:6])
    n = gone.shape[0]
    for wm in (0, 1, n // 2, n - 1, n):
        m = dev()
        m.insert(steps[0][1], steps[0][2], steps[0][3], None)
        assert m.clear_rays(*steps[1][1:6], wm) == (int(gone.sum()), n - int(gone.sum()), int((~gone[:wm]).sum()))


def test_a_clearing_that_removes_nothing_does_not_show(made):
    """the map downloads byte-equal, and every later fold equals that of a map that was never cleared"""
    dev, _ = made
    a, b = dev(), dev()
    for f in range(3):
        pts = E.gaussian(1025, 40 + f)
        R, t = E.random_pose(f)
        words = np.arange(1025, dtype=np.uint32)
        assert a.insert(pts, R, t, words) == b.insert(pts, R, t, words)
        assert a.clear_rays(pts * 0.01, R, t, np.zeros(3), 0.0, 7)[0::2] == (0, 7)  # (rays shorter than a voxel: nothing walked)
        assert a.rows().tobytes() == b.rows().tobytes() and a.words().tobytes() == b.words().tobytes()


def test_two_maps_interleaved(made):
    dev, _ = made
    a, b = dev(), dev(voxel=0.25)
    steps, want = Cl.expected("size-1025-1025")
    R, t = E.random_pose(3)
    other = E.gaussian(3000, 77)
    b.insert(other, R, t, np.arange(3000, dtype=np.uint32))
    b_rows, b_words = b.rows().tobytes(), b.words().tobytes()
    for step, (ans, rows, words) in zip(steps, want):
        got = a.insert(step[1], step[2], step[3], np.arange(step[1].shape[0], dtype=np.uint32)) if step[0] == "fold" else a.clear_rays(*step[1:])
        assert tuple(got) == tuple(ans) and a.rows().tobytes() == rows.tobytes()
        assert b.rows().tobytes() == b_rows and b.words().tobytes() == b_words  # clearing one leaves the other's bytes alone
    ref = Cl.RefClearMap(0.25)
    ref.insert(other, R, t, np.arange(3000, dtype=np.uint32))
    want_b = ref.clear_rays(other * 1.5, R, t, np.zeros(3), 0.0, 100)
    assert b.clear_rays(other * 1.5, R, t, np.zeros(3), 0.0, 100) == want_b and want_b[0] > 0 and E.same_bits(b.rows(), ref.rows())
    assert a.rows().tobytes() == want[-1][1].tobytes()


def test_determinism(made):
    dev, _ = made
    first, second = dev(initial_rows=1), dev(initial_rows=1)
    Cl.replay("size-4097-257", first)
    Cl.replay("size-4097-257", second)
    assert first.rows().tobytes() == second.rows().tobytes() and first.words().tobytes() == second.words().tobytes()


def test_a_map_much_larger_than_any_cloud(natives, made):
    """20 480 rows from clouds of 256 points in a context of the test's own, which has never seen a larger cloud: flags, marks or a
    scan laid over the builder's scratch (sized by the largest cloud) would write past it"""
    _, twin = made
    own = capi.Context(0)
    try:
        m = DevImpl(own, initial_rows=1, **TWIN)
        try:
            want = Cl.replay("large", m, also=(twin(initial_rows=1),))
            assert want[79][0] == (256, 20480) and want[80][0][0] > 100 and want[81][0][0] > 0
        finally:
            m.close()
    finally:
        own.close()


def test_the_scene(made):
    """fold, fold, clear: no row inside the box, every wall row of frame 1 still there (tests/test_host_map_clear.py confirms both
    on the restatement)"""
    dev, twin = made
    m = dev()
    Cl.replay("scene", m, also=(twin(),))
    _, hits_box, frame1, _ = Cl.scene()
    rows = m.rows()
    assert not ((np.abs(rows[:, 0] - 6.0) < 0.25) & (np.abs(rows[:, 1]) < 1.0) & (np.abs(rows[:, 2]) < 0.6)).any()
    first = Cl.RefClearMap(Cl.VOXEL)
    first.insert(frame1, *E.IDENTITY)
    wall_rows = first.rows()[first.rows()[:, 0] > 9.0]
    have = set(map(bytes, rows.view(np.uint8).reshape(-1, 12)))
    assert wall_rows.shape[0] > 50 and all(bytes(r) in have for r in wall_rows.view(np.uint8).reshape(-1, 12))


def _clear(h, mid, cid, R, t, o, margin, wm, a, b, k):
    p = lambda v: None if v is None else v.ctypes.data_as(_dp)  # noqa: E731
    r = lambda v: None if v is None else C.byref(v)  # noqa: E731
    return capi.hip_lib().madicp_map_clear_rays(h, mid, cid, p(R), p(t), p(o), margin, wm, r(a), r(b), r(k))


def test_refusals(ctx, made):
    dev, _ = made
    m = dev()
    R, t = np.eye(3).reshape(9), np.zeros(3)
    pts = E.gaussian(500, 9)
    rows = m.insert(pts, R, t, np.arange(500, dtype=np.uint32))[1]
    before, before_w = m.rows().tobytes(), m.words().tobytes()
    rays, o = E.gaussian(300, 10) * 3.0, np.zeros(3)
    cid = ctx.cloud_upload(rays)
    try:
        a, b, k = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
        ok = (ctx._h, m.mid, cid, R, t, o, 0.0, 0, a, b, k)
        for i in (0, 3, 4, 5, 8, 9, 10):  # every pointer
            assert _clear(*[None if j == i else v for j, v in enumerate(ok)]) == INVALID
        assert _clear(ctx._h, m.mid + 1000, cid, R, t, o, 0.0, 0, a, b, k) == INVALID  # unknown map
        assert _clear(ctx._h, m.mid, cid + 1000, R, t, o, 0.0, 0, a, b, k) == INVALID  # unknown cloud
        for bad in (np.nan, np.inf, -np.inf):
            for which in (3, 4, 5):
                args = list(ok)
                args[which] = args[which].copy()
                args[which][2] = bad
                assert _clear(*args) == INVALID
            assert _clear(ctx._h, m.mid, cid, R, t, o, bad, 0, a, b, k) == INVALID
        assert _clear(ctx._h, m.mid, cid, R, t, o, -0.5, 0, a, b, k) == INVALID
        assert _clear(ctx._h, m.mid, cid, R, t, o, 0.0, -1, a, b, k) == INVALID
        assert _clear(ctx._h, m.mid, cid, R, t, o, 0.0, rows + 1, a, b, k) == INVALID
        assert (a.value, b.value, k.value) == (-7, -7, -7) and ctx.map_size(m.mid) == rows
        assert m.rows().tobytes() == before and m.words().tobytes() == before_w
        # an empty map answers without a launch (a resident cloud always holds a point: the empty cloud is the host twin's case)
        empty = dev()
        assert ctx.map_clear_rays(empty.mid, cid, R, t) == (0, 0, 0) and _clear(ctx._h, empty.mid, cid, R, t, o, 0.0, 1, a, b, k) == INVALID
        # the clearing does not touch the builder's scratch: it is legal while a look-ahead build is in flight, the build is unharmed,
        # and the cloud is only read
        ctx.tree_build_begin(E.gaussian(3000, 10), 0.2, 0.1)
        try:
            got = ctx.map_clear_rays(m.mid, cid, R, t, o, 0.1, rows)
        finally:
            tid, leaves = ctx.tree_build_end()
            ctx.tree_release(tid)
        ref = Cl.RefClearMap(Cl.VOXEL)
        ref.insert(pts, R, t, np.arange(500, dtype=np.uint32))
        assert got == ref.clear_rays(rays, R, t, o, 0.1, rows) and got[0] > 0 and leaves > 0
        assert E.same_bits(m.rows(), ref.rows()) and m.words().tobytes() == ref.attr().tobytes()
        assert ctx.cloud_download(cid).tobytes() == np.ascontiguousarray(rays).tobytes()
    finally:
        ctx.cloud_release(cid)
