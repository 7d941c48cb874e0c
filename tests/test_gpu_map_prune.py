"""Context.map_prune (madicp_map_prune: fe::map_prune_mark / the tile scan over the prune's own buffers / fe::map_compact / the
memset and fe::map_rehash) against BOTH the numpy restatement of tests/map_prune_ref.py and the host twin, bit for bit after
EVERY step of the shared sequences: row counts around the wavefront, the workgroup and the 1 024-mark scan tile, the four kinds
of radius, the boundary, growth, the attribute column, a map far larger than any cloud its context has seen, every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloud_export_ref as E
import map_prune_ref as P
from mad_icp_amd import capi
from map_impls import DevImpl, maps  # noqa: F401 (maps is a fixture)
from test_host_map_prune import TWIN

pytestmark = pytest.mark.gpu

INVALID = -1
_dp = C.POINTER(C.c_double)


@pytest.fixture
def made(ctx, maps):
    """device map / host twin factories"""
    return functools.partial(maps.dev, ctx, **TWIN), functools.partial(maps.host, **TWIN)


@pytest.mark.parametrize("name", P.SIZE_NAMES)
def test_sizes_and_radii(made, name):
    dev, twin = made
    want = P.replay(name, dev(), also=(twin(),))
    assert want[0][0][1] == int(name.split("-")[1])  # rows == M: the prune's kernels see exactly that many


@pytest.mark.parametrize("name", P.OTHER_NAMES)
def test_sequences(made, name):
    dev, twin = made
    P.replay(name, dev(), also=(twin(),))


def test_boundary_rows(made):
    dev, _ = made
    m = dev()
    P.replay("boundary", m)
    assert m.rows().tolist() == [[3.0, 4.0, 0.0], [0.0, 0.0, 5.0], [-5.0, 0.0, 0.0]] and m.words().tolist() == [0, 1, 4]


def test_watermarks(made):
    dev, _ = made
    steps, _ = P.expected("reentry")
    keep = P.RefPruneMap(P.VOXEL)
    keep.insert(steps[0][1], steps[0][2], steps[0][3])
    mask = keep.kept_mask(steps[1][1], steps[1][2])
    n = mask.shape[0]
    for wm in (0, 1, n // 2, n - 1, n):
        m = dev()
        m.insert(steps[0][1], steps[0][2], steps[0][3], None)
        assert m.prune(steps[1][1], steps[1][2], wm) == (n - int(mask.sum()), int(mask.sum()), int(mask[:wm].sum()))


def test_growth_on_both_sides(made):
    """initial_rows = 1 (grows, and is pruned between growths) against a map created large: byte-equal after every step"""
    dev, twin = made
    small, large = dev(initial_rows=1), dev(initial_rows=1 << 16)
    steps, want = P.expected("growth")
    assert sum(1 for s in steps if s[0] == "fold") == 6 and want[-1][1].shape[0] > 0
    for step, (ans, rows, words) in zip(steps, want):
        for m in (small, large):
            got = m.insert(step[1], step[2], step[3], np.arange(4097, dtype=np.uint32)) if step[0] == "fold" else m.prune(*step[1:])
            assert tuple(got) == tuple(ans)
        assert small.rows().tobytes() == large.rows().tobytes() == rows.tobytes()
        assert small.words().tobytes() == large.words().tobytes() == words.tobytes()


def test_attribute_column_follows_and_does_not_show(made):
    """attr[j] is the word of the row that now sits at j (the point's index: the restatement's); the rows equal those of a map
    without the column on the same steps"""
    dev, _ = made
    with_col, without = dev(initial_rows=1), dev(initial_rows=1, with_attr=False)
    want = P.replay("posed", with_col, also=(without,))
    assert with_col.rows().tobytes() == without.rows().tobytes() and len(set(want[-1][2].tolist())) > 100


def test_two_maps_interleaved(made):
    dev, _ = made
    a, b = dev(), dev(voxel=0.25)
    steps, want = P.expected("posed")
    R, t = E.random_pose(3)
    other = E.gaussian(3000, 77)
    b.insert(other, R, t, np.arange(3000, dtype=np.uint32))
    b_rows, b_words = b.rows().tobytes(), b.words().tobytes()
    for step, (ans, rows, words) in zip(steps, want):
        got = a.insert(step[1], step[2], step[3], np.arange(step[1].shape[0], dtype=np.uint32)) if step[0] == "fold" else a.prune(*step[1:])
        assert tuple(got) == tuple(ans) and a.rows().tobytes() == rows.tobytes()
        assert b.rows().tobytes() == b_rows and b.words().tobytes() == b_words  # pruning one leaves the other's bytes alone
    removed, left, _ = b.prune(t, 10.0, 0)
    assert removed > 0 and left > 0 and a.rows().tobytes() == want[-1][1].tobytes()


def test_determinism(made):
    dev, _ = made
    first, second = dev(initial_rows=1), dev(initial_rows=1)
    P.replay("growth", first)
    P.replay("growth", second)
    assert first.rows().tobytes() == second.rows().tobytes() and first.words().tobytes() == second.words().tobytes()


def test_a_prune_that_removes_nothing_does_not_show(made):
    dev, _ = made
    a, b = dev(), dev()
    for f in range(3):
        pts = E.gaussian(1025, 40 + f)
        R, t = E.random_pose(f)
        words = np.arange(1025, dtype=np.uint32)
        assert a.insert(pts, R, t, words) == b.insert(pts, R, t, words)
        assert a.prune(np.zeros(3), 1.0e5, 7)[0::2] == (0, 7)
        assert a.rows().tobytes() == b.rows().tobytes() and a.words().tobytes() == b.words().tobytes()


def test_the_key_is_the_stored_one(made):
    dev, _ = made
    R, t = E.IDENTITY
    below, exact = np.array([[np.nextafter(0.5, 0.0), 0.25, 0.25]]), np.array([[0.5, 0.25, 0.25]])
    far = np.array([[40.0, 0.25, 0.25]])
    m = dev(voxel=0.5)
    for pts in (below, exact, far):
        assert m.insert(pts, R, t, None)[0] == 1
    assert m.prune(np.zeros(3), 10.0, 3) == (1, 2, 2)
    assert m.insert(below, R, t, None) == (0, 2) and m.insert(exact, R, t, None) == (0, 2) and m.insert(far, R, t, None) == (1, 3)


def test_a_map_much_larger_than_any_cloud(natives, made):
    """20 480 rows from clouds of 256 points in a context of the test's own, which has never seen a larger cloud: a scan run over
    the builder's scratch (sized by the largest cloud) would write past it"""
    _, twin = made
    own = capi.Context(0)
    try:
        m = DevImpl(own, initial_rows=1, **TWIN)
        try:
            want = P.replay("large", m, also=(twin(initial_rows=1),))
            assert want[79][0] == (256, 20480) and 2000 < want[80][0][1] < 18000 and want[82][0][0] > 0
        finally:
            m.close()
    finally:
        own.close()


def _prune(ctx_h, mid, c, r, wm, a, b, k):
    return capi.hip_lib().madicp_map_prune(ctx_h, mid, None if c is None else c.ctypes.data_as(_dp), r, wm, None if a is None else C.byref(a),
                                           None if b is None else C.byref(b), None if k is None else C.byref(k))


def test_refusals(ctx, made):
    dev, _ = made
    m = dev()
    R, t = E.IDENTITY
    rows = m.insert(E.gaussian(500, 9), R, t, np.arange(500, dtype=np.uint32))[1]
    before, before_w = m.rows().tobytes(), m.words().tobytes()
    c = np.zeros(3)
    a, b, k = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    h, mid = ctx._h, m.mid
    assert _prune(None, mid, c, 1.0, 0, a, b, k) == INVALID
    assert _prune(h, mid, None, 1.0, 0, a, b, k) == INVALID
    assert _prune(h, mid, c, 1.0, 0, None, b, k) == INVALID and _prune(h, mid, c, 1.0, 0, a, None, k) == INVALID
    assert _prune(h, mid, c, 1.0, 0, a, b, None) == INVALID
    assert _prune(h, mid + 1000, c, 1.0, 0, a, b, k) == INVALID
    for bad in (np.nan, np.inf, -np.inf):
        cb = c.copy()
        cb[2] = bad
        assert _prune(h, mid, cb, 1.0, 0, a, b, k) == INVALID
        assert _prune(h, mid, c, bad, 0, a, b, k) == INVALID
    for r in (0.0, -1.0, 1e200):  # (1e200: finite, its square is not)
        assert _prune(h, mid, c, r, 0, a, b, k) == INVALID
    assert _prune(h, mid, c, 1.0, -1, a, b, k) == INVALID and _prune(h, mid, c, 1.0, rows + 1, a, b, k) == INVALID
    assert (a.value, b.value, k.value) == (-7, -7, -7) and ctx.map_size(mid) == rows
    assert m.rows().tobytes() == before and m.words().tobytes() == before_w
    empty = dev()
    assert empty.prune(c, 1.0, 0) == (0, 0, 0) and _prune(h, empty.mid, c, 1.0, 1, a, b, k) == INVALID
    # the prune does not touch the builder's scratch: it is legal while a look-ahead build is in flight, and the build is unharmed
    ctx.tree_build_begin(E.gaussian(3000, 10), 0.2, 0.1)
    try:
        removed, left, mark = m.prune(c, 8.0, rows)
    finally:
        tid, leaves = ctx.tree_build_end()
        ctx.tree_release(tid)
    ref = P.RefPruneMap(P.VOXEL)
    ref.insert(E.gaussian(500, 9), R, t, np.arange(500, dtype=np.uint32))
    assert (removed, left, mark) == ref.prune(c, 8.0, rows) and removed > 0 and leaves > 0
    assert E.same_bits(m.rows(), ref.rows()) and m.words().tobytes() == ref.attr().tobytes()
