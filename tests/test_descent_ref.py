"""tests/descent_ref.py held to the oracle BIT FOR BIT (no GPU): the numpy restatement of the descent and of one
MADicp::update walks `O.export_to_nodes(tree.export())` and must give what the oracle gives on its own trees — leaf
ordinals and depths of `O.Tree.search`, ordinals / gate / matched flags / depth sum of `O.icp_linearize`, H and b within
the suite's bar (1e-10 of max|H|, tests/test_gpu_baseline_configs.py check_linearize) — on the street problems, the
four-walls clouds and the sixty random small clouds of tests/test_gpu_edge_parity.py, with NaN / inf rows, queries exactly on
a split plane (s == 0: right) and their floating-point neighbours.  This is what lets tests/test_gpu_default_path_parity.py
use the module as THE reference on node arrays the oracle cannot walk (trees built and transformed on the device).

Also here, because anyone can reproduce them without a GPU: the yield of the plane-hugging query construction (at least
2 000 queries within 1e-12 of a visited plane, at least 50 exactly on one) and, printed, the histogram of the smallest |s|
a pair of the bench problem meets on its way down (how many decisions sit within 1e-13 ... 1e-3 m of a split plane)."""
import os

import numpy as np
import pytest

import descent_ref as D
import oracle_lib as O
from fixtures import B_MAX, B_MIN, B_RATIO, RHO_KER, four_walls, street_problem

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def nodes_of(tree):
    return O.export_to_nodes(tree.export())[0]


def special_queries(nodes, rng):
    """NaN / inf rows, every (sampled) internal node's own centroid (s == 0 exactly where the descent reaches it) with its
    nextafter neighbours in every coordinate, and the plane-hugging construction."""
    internal = np.flatnonzero(nodes["right"] != 0)
    out = [np.array([[np.nan, 0.0, 0.0], [0.0, np.nan, 1.0], [np.nan] * 3, [np.inf, 0.0, 0.0], [1.0, -np.inf, 2.0],
                     [np.inf, -np.inf, np.inf], [0.0, 0.0, 0.0], [1e300, 1e300, -1e300]])]
    if internal.size:
        m = nodes["mean"][rng.choice(internal, min(400, internal.size), replace=False)]
        out.append(m)
        for c in range(3):
            for sign in (-np.inf, np.inf):
                q = m.copy()
                q[:, c] = np.nextafter(q[:, c], sign)
                out.append(q)
        out.append(D.plane_hugging_queries(nodes, rng, 40)[0])
    return np.concatenate(out)


def check_search(tree, q):
    nodes = nodes_of(tree)
    leaf, depth, dist = tree.search(q, want_dist=True)
    d = D.descend(nodes, q)
    assert np.array_equal(d["leaf"], leaf)
    assert np.array_equal(d["depth"], depth)
    assert np.array_equal(D.nn_dist(nodes, d["node"], q), dist, equal_nan=True)
    return d


def check_linearize(moving, fixed, T, b_max):
    nodes = nodes_of(fixed)
    H, b, corr, rej, mat, depth = O.icp_linearize(moving, fixed, T, b_max, RHO_KER, B_RATIO)
    r = D.linearize(nodes, moving.leaves()[0], T, b_max, RHO_KER, B_RATIO)
    assert np.array_equal(r["ordinal"], corr)
    assert np.array_equal(r["rejected"], rej)
    assert np.array_equal(r["matched"], mat)
    assert int(r["depth"].sum()) == depth
    assert np.allclose(np.asarray(r["H"], np.float64), H, rtol=0, atol=1e-10 * max(np.abs(H).max(), 1e-300))
    assert np.allclose(np.asarray(r["b"], np.float64), b, rtol=0, atol=1e-10 * max(1.0, np.abs(b).max()))
    return r


@pytest.mark.parametrize("K", [2, 3])
def test_street_problem_bit_for_bit(K):
    pb = street_problem(K)
    gold = np.load(os.path.join(GOLD, "street_k%d.npz" % (3 if K == 3 else 1)))
    q = O.Tree(pb["query_scans"][0], B_MAX, B_MIN, 2)
    T0 = pb["query_guess"][0]
    poses = [T0, O.pose44(gold["X_iters"][5]), O.pose44(gold["X_iters"][14])]
    rng = np.random.default_rng(100 + K)
    n_zero = n_matched = 0
    for s, Tk in zip(pb["keyframe_scans"], pb["keyframe_poses"]):
        t = O.Tree(s, B_MAX, B_MIN, 2)
        t.transform(Tk[:3, :3], Tk[:3, 3])
        nodes = nodes_of(t)
        scan_in_map = pb["query_scans"][0] @ T0[:3, :3].T + T0[:3, 3]
        d = check_search(t, np.concatenate([scan_in_map, special_queries(nodes, rng)]))
        n_zero += int((d["min_abs_s"] == 0.0).sum())
        for T in poses:
            n_matched += int(check_linearize(q, t, T, B_MAX)["matched"].sum())
    assert n_zero >= 50          # queries exactly ON a split plane were among them (they go right)
    assert n_matched > 1000      # ... and pairs that pass the gate, so H and b were compared on real terms


def test_a_query_on_the_plane_goes_right():
    """s == 0 is not < 0: the root's own centroid descends into the root's RIGHT sub-tree, in the oracle and here."""
    pb = street_problem(2)
    t = O.Tree(pb["keyframe_scans"][0], B_MAX, B_MIN, 2)
    nodes = nodes_of(t)
    q = nodes["mean"][:1].copy()
    d = check_search(t, q)
    assert d["min_abs_s"][0] == 0.0
    assert d["node"][0] >= nodes["right"][0]
    w, sa, sb = D.parting(nodes, nodes, q)
    assert w[0] == -1 and np.isnan(sa[0]) and np.isnan(sb[0])
    # parting finds a moved plane: the root's centroid pushed along its normal so that the same query falls left
    moved = nodes.copy()
    moved["mean"][0] += 1e-3 * moved["dir"][0]
    w, sa, sb = D.parting(nodes, moved, q)
    assert w[0] == 0 and sa[0] == 0.0 and sb[0] < 0.0


@pytest.mark.parametrize("b_max", [1e-5, B_MAX])
def test_four_walls_bit_for_bit(b_max):
    np.random.seed(42)
    cloud = four_walls(2000)
    t = O.Tree(cloud, b_max, 0.1, 2)
    rng = np.random.default_rng(9)
    q = cloud[rng.integers(0, len(cloud), 5000)] + rng.normal(0, 0.05, (5000, 3))
    check_search(t, np.concatenate([q, cloud[:2000], special_queries(nodes_of(t), rng)]))
    T = np.eye(4)
    T[:3, :3] = [[np.cos(0.1), -np.sin(0.1), 0.0], [np.sin(0.1), np.cos(0.1), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.05, -0.02, 0.01]
    for pose in (np.eye(4), T):
        check_linearize(t, t, pose, max(b_max, 0.05))


def test_sixty_random_small_clouds_bit_for_bit():
    """The clouds of tests/test_gpu_edge_parity.py::test_random_small_clouds_nearest_neighbour_and_linearisation, drawn the
    same way: trees of one, two, three leaves, duplicates, lines, leaves without a normal of their own."""
    r2 = np.random.default_rng(77)
    rng = np.random.default_rng(78)
    for i in range(60):
        n = int(r2.integers(1, 400))
        kind = int(r2.integers(4))
        c = r2.normal(size=(n, 3)) * r2.choice([0.01, 0.3, 5.0], size=3)
        if kind == 1:
            c[:, 2] = 0.0
        elif kind == 2:
            c[:, 1:] = 0.0
        elif kind == 3:
            c = np.repeat(c[: max(1, n // 4)], 4, axis=0)
        c = c + r2.normal(size=3) * 10.0
        b_max, b_min = float(r2.choice([1e-5, 0.05, 0.2, 1.0])), float(r2.choice([0.01, 0.1, 0.5]))
        par = int(r2.integers(3))
        ot = O.Tree(c, b_max, b_min, par)
        q = c + r2.normal(size=c.shape) * 0.01
        check_search(ot, np.concatenate([q, special_queries(nodes_of(ot), rng)]))
        T0 = np.eye(4)
        T0[:3, 3] = r2.normal(size=3) * 0.02
        check_linearize(ot, ot, T0, b_max)


def test_plane_hugging_construction_yield():
    """The condition that keeps the plane-hugging part of tests/test_gpu_default_path_parity.py honest, shown here on an
    oracle tree: the construction reaches at least 2 000 queries within 1e-12 of a VISITED split plane and at least 50
    exactly on one — and on every one of them this module and the oracle agree."""
    pb = street_problem(2)
    t = O.Tree(pb["keyframe_scans"][0], B_MAX, B_MIN, 2)
    q, _ = D.plane_hugging_queries(nodes_of(t), np.random.default_rng(3), 400, repeats=4)
    d = check_search(t, q)
    near, on = int((d["min_abs_s"] < 1e-12).sum()), int((d["min_abs_s"] == 0.0).sum())
    assert near >= 2000 and on >= 50, (q.shape[0], near, on)


def test_levels_and_subtree_sizes():
    pb = street_problem(2)
    t = O.Tree(pb["keyframe_scans"][0], B_MAX, B_MIN, 2)
    ex = t.export()
    nodes = nodes_of(t)
    size = D.subtree_sizes(nodes)
    internal = np.flatnonzero(nodes["right"] != 0)
    assert size[0] == nodes.shape[0]
    assert np.array_equal(size[internal + 1], nodes["right"][internal] - 1)     # the left sub-tree ends where the right begins
    lev = D.levels(nodes)
    assert np.array_equal(lev[internal + 1], lev[internal] + 1) and np.array_equal(lev[internal + nodes["right"][internal]], lev[internal] + 1)
    # the oracle's member counts add up along the same structure
    assert np.array_equal(ex["num_points"][internal], ex["num_points"][internal + 1] + ex["num_points"][internal + nodes["right"][internal]])


def test_min_abs_s_histogram_of_the_bench_problem(capsys):
    """The CPU-side figure next to the census of tests/test_gpu_default_path_parity.py: of the bench problem's pairs
    (synth.make_problem(16, seed=1), every moving leaf against every keyframe tree at the guess) how many pass within
    1e-13 ... 1e-3 m of a split plane on their way down.  A builder whose node errors are e moves decisions only among the
    pairs counted under e: the census's N scales with this column."""
    from mad_icp_amd import synth

    pb = synth.make_problem(16, seed=1, n_queries=1)
    q = O.Tree(pb["query_scans"][0], B_MAX, B_MIN, 3)
    p = q.leaves()[0]
    T0 = pb["query_guess"][0]
    edges = 10.0 ** np.arange(-13, -2)
    counts, pairs = np.zeros(edges.size, np.int64), 0
    for s, Tk in zip(pb["keyframe_scans"], pb["keyframe_poses"]):
        t = O.Tree(s, B_MAX, B_MIN, 3)
        t.transform(Tk[:3, :3], Tk[:3, 3])
        r = D.linearize(nodes_of(t), p, T0, B_MAX, RHO_KER, B_RATIO)
        counts += (r["min_abs_s"][:, None] < edges[None, :]).sum(axis=0)
        pairs += p.shape[0]
    with capsys.disabled():
        print("\n[min |s| on the way down, bench problem at the guess] %d pairs; within " % pairs
              + ", ".join("%.0e m: %d" % (e, c) for e, c in zip(edges, counts)))
    assert pairs > 300000 and (np.diff(counts) >= 0).all()
    assert counts[-1] > 0     # (pairs within a micrometre of a plane exist: the census has something to count)
