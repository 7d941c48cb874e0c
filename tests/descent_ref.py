"""A plain numpy restatement of the reference's descent and of one MADicp::update that can walk ANY node array.

TEST INFRASTRUCTURE ONLY (a helper like oracle_lib.py).  The oracle (oracle_lib.py) walks only the trees it built itself;
this module walks the 64-byte `capi.NODE_DTYPE` array of include/madicp_hip.h whoever made it — the oracle's export, the host
builder, or a tree built and transformed on the device and downloaded again: left child = i + 1, right child = i + `right`,
a leaf iff `right == 0`.  Everything is float64 in the oracle's operation order (oracle/linalg.h): numpy's element-wise
arithmetic rounds every product and sum on its own (no fused multiply-add), which is what the oracle's build does.
tests/test_descent_ref.py holds it to the oracle bit for bit; that is what makes it a reference and not a third opinion.

  dotc(a, b) = (a0*b0 + a1*b1) + a2*b2          the contiguous / packet order (linalg.h:47-52)
  dots(a, b) = a0*b0 + (a1*b1 + a2*b2)          the strided / scalar order   (linalg.h:43-45)
"""
import numpy as np


def dotc(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def dots(a, b):
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def mul(R, x):
    """Matrix3d * Vector3d, rows in the `dots` order (linalg.h:78-82); x: (..., 3)."""
    R = np.asarray(R, dtype=np.float64)
    return np.stack([R[i, 0] * x[..., 0] + (R[i, 1] * x[..., 1] + R[i, 2] * x[..., 2]) for i in range(3)], axis=-1)


def side(nodes, at, q):
    """s = dotc(q - mean, dir) of the nodes `at` for the queries q (one node per query)."""
    return dotc(q - nodes["mean"][at], nodes["dir"][at])


def walk(nodes, q):
    """The descent of mad_oracle.cpp:157-166, level by level.  Yields (idx, at, s) per level: the queries still above a leaf, the
    internal node each one stands at, and s there; the caller may read `cur` (the node every query stands at) afterwards via
    the generator's return value.  Left iff s < 0: NaN compares false and goes right."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    right = nodes["right"].astype(np.int64)
    cur = np.zeros(q.shape[0], np.int64)
    idx = np.arange(q.shape[0])
    while True:
        idx = idx[right[cur[idx]] != 0]
        if idx.size == 0:
            return cur
        at = cur[idx]
        with np.errstate(invalid="ignore", over="ignore"):
            s = side(nodes, at, q[idx])
            left = s < 0.0
        cur[idx] = np.where(left, at + 1, at + right[at])
        yield idx, at, s


def descend(nodes, q):
    """-> dict(node, leaf, depth, min_abs_s) per query: the index of the leaf's node, its getLeafs() ordinal, the number of
    internal nodes visited and the smallest |s| met on the way (inf for a single-leaf tree; a NaN s is not counted)."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    depth = np.zeros(q.shape[0], np.int32)
    mins = np.full(q.shape[0], np.inf)
    g = walk(nodes, q)
    while True:
        try:
            idx, _, s = next(g)
        except StopIteration as stop:
            cur = stop.value
            break
        depth[idx] += 1
        mins[idx] = np.fmin(mins[idx], np.abs(s))
    return dict(node=cur, leaf=nodes["leaf_id"][cur].astype(np.uint32), depth=depth, min_abs_s=mins)


def nn_dist(nodes, at, q):
    """norm(q - leaf.mean) as searchCloud reports it (oracle_capi.cpp: sqrt(dotc(d, d)))."""
    d = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3) - nodes["mean"][at]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(dotc(d, d))


def linearize(nodes, moving_means, T, b_max, rho_ker, b_ratio):
    """One MADicp::update (mad_oracle.cpp:214-267) of the moving leaf means against the tree `nodes` at pose T (4x4 or 3x4).
    -> dict(ordinal, rejected, depth (per leaf), matched, H (6,6), b (6), node, min_abs_s, ml).  H and b are accumulated in
    np.longdouble (they are only ever compared to a tolerance); every per-pair quantity is the oracle's bit for bit."""
    T = np.asarray(T, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    p = np.ascontiguousarray(moving_means, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ml = t + mul(R, p)                                    # apply(): t + R p, the product in the `dots` order
        d = descend(nodes, ml)
        f = d["node"]
        fp, fn, bbox0 = nodes["mean"][f], nodes["dir"][f], nodes["bbox0"][f]
        diff = ml - fp
        src_ball = b_max + b_ratio * np.sqrt(dotc(p, p))
        rejected = np.sqrt(dotc(diff, diff)) > src_ball       # NaN compares false: not rejected
        keep = ~rejected
        e = dotc(diff, fn)
        J = np.empty((p.shape[0], 6))
        for j in range(3):
            J[:, j] = dotc(fn, R[:, j])
        neg = -J[:, :3]
        z = np.zeros(p.shape[0])
        S = (np.stack([z, p[:, 2], -p[:, 1]], 1), np.stack([-p[:, 2], z, p[:, 0]], 1), np.stack([p[:, 1], -p[:, 0], z], 1))
        for j in range(3):
            J[:, 3 + j] = dotc(neg, S[j])
        rho = np.sqrt(rho_ker)
        chi = np.abs(e)
        scale = np.where(chi > rho, rho / chi, 1.0)
        w = 1.0 - bbox0 / b_max
        scale = scale * (w * w)
        sJ = scale[:, None] * J
        Hp = (sJ[keep][:, :, None] * J[keep][:, None, :])
        bp = sJ[keep] * e[keep][:, None]
        H = Hp.sum(axis=0, dtype=np.longdouble)
        b = bp.sum(axis=0, dtype=np.longdouble)
    return dict(ordinal=d["leaf"], rejected=rejected.astype(np.uint8), depth=d["depth"], matched=keep.astype(np.uint8),
                H=H, b=b, node=f, min_abs_s=d["min_abs_s"], ml=ml)


def parting(nodes_a, nodes_b, q):
    """Two arrays with identical `right` links: per query the first node index where the two descents take different sides
    (-1 if they never do), and s there under both arrays (NaN where they never part)."""
    assert np.array_equal(nodes_a["right"], nodes_b["right"])
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    n = q.shape[0]
    right = nodes_a["right"].astype(np.int64)
    cur = np.zeros(n, np.int64)
    where = np.full(n, -1, np.int64)
    sa, sb = np.full(n, np.nan), np.full(n, np.nan)
    idx = np.arange(n)
    while True:
        idx = idx[right[cur[idx]] != 0]
        if idx.size == 0:
            return where, sa, sb
        at = cur[idx]
        with np.errstate(invalid="ignore", over="ignore"):
            a, b = side(nodes_a, at, q[idx]), side(nodes_b, at, q[idx])
            la, lb = a < 0.0, b < 0.0
        part = la != lb
        where[idx[part]], sa[idx[part]], sb[idx[part]] = at[part], a[part], b[part]
        idx, at, la = idx[~part], at[~part], la[~part]
        cur[idx] = np.where(la, at + 1, at + right[at])


def levels(nodes):
    """Depth of every node of the preorder array (root 0)."""
    right = nodes["right"].astype(np.int64)
    lev = np.zeros(nodes.shape[0], np.int32)
    front = np.array([0], np.int64)
    while front.size:
        front = front[right[front] != 0]
        kids = np.concatenate([front + 1, front + right[front]])
        lev[kids] = np.concatenate([lev[front], lev[front]]) + 1
        front = kids
    return lev


def subtree_sizes(nodes):
    """Number of nodes of the sub-tree rooted at every node (a leaf: 1)."""
    right = nodes["right"].astype(np.int64)
    lev = levels(nodes)
    size = np.ones(nodes.shape[0], np.int64)
    for l in range(int(lev.max()) - 1, -1, -1):
        i = np.flatnonzero((lev == l) & (right != 0))
        size[i] = 1 + size[i + 1] + size[i + right[i]]
    return size


def plane_hugging_queries(nodes, rng, per_level, repeats=1, steps=(1, 2, 3)):
    """Queries within rounding of a split plane: for up to `per_level` internal nodes drawn at every depth (each taken
    `repeats` times, with a leaf mean of its own every time), a leaf mean p of the node's sub-tree projected on the node's
    plane, q = p - s n, and the neighbours `nextafter` gives in the largest component of n, 1, 2, 3 steps each way.
    -> (queries (7 m, 3), the node each one was aimed at (7 m,))."""
    right = nodes["right"].astype(np.int64)
    lev, size = levels(nodes), subtree_sizes(nodes)
    leaf_rows = np.flatnonzero(right == 0)
    pick = []
    for l in range(int(lev.max()) + 1):
        i = np.flatnonzero((lev == l) & (right != 0))
        if i.size > per_level:
            i = rng.choice(i, per_level, replace=False)
        pick.append(i)
    at = np.sort(np.tile(np.concatenate(pick), repeats))
    lo = np.searchsorted(leaf_rows, at)
    hi = np.searchsorted(leaf_rows, at + size[at])
    p = nodes["mean"][leaf_rows[lo + (rng.random(at.size) * (hi - lo)).astype(np.int64)]]
    m, n = nodes["mean"][at], nodes["dir"][at]
    ok = np.isfinite(p).all(axis=1) & np.isfinite(m).all(axis=1) & np.isfinite(n).all(axis=1)
    at, p, m, n = at[ok], p[ok], m[ok], n[ok]
    q0 = p - dotc(p - m, n)[:, None] * n
    c = np.abs(n).argmax(axis=1)
    rows = np.arange(at.size)
    out = [q0]
    for sign in (-np.inf, np.inf):
        q = q0.copy()
        for k in range(max(steps)):
            q = q.copy()
            q[rows, c] = np.nextafter(q[rows, c], sign)
            if k + 1 in steps:
                out.append(q)
    return np.concatenate(out), np.tile(at, len(out))
