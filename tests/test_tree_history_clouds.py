"""The clouds of tests/tree_history_clouds.py are what they are said to be — held with the HOST builder, no GPU.

tests/test_gpu_tree_build_history.py builds pairs of these clouds on one device context so that the second build takes a
wrong hint from the first.  Whether the hint IS wrong is a property of the two trees: their depths, their leaf counts, the
leaves under the nodes of one level.  Everything that file relies on is asserted here."""
import numpy as np
import pytest

import tree_history_clouds as Cl


@pytest.fixture(scope="module")
def trees(natives):
    cache = {}

    def get(cloud):
        if cloud.name not in cache:
            t = Cl.host_tree(cloud)
            cache[cloud.name] = (t.nodes.copy(), t.num_leaves)
        return cache[cloud.name]

    return get


def test_the_two_integer_rules():
    assert Cl.leaf_cap(4000, 1000) == 1381
    assert Cl.leaf_cap(40000, 1) == 257
    assert Cl.leaf_cap(4000, 40000) == 4000
    assert [Cl.similar(n, 4000) for n in Cl.HEADS] == [False, True, True, False]
    assert not Cl.similar(4000, 0) and Cl.similar(1, 1) and not Cl.similar(141, 4000) and not Cl.similar(4000, 141)
    assert [Cl.first_steps(d) for d in (-1, 0, 14, 16, 17, 18, 29, 94)] == [20, 18, 18, 18, 19, 20, 20, 20]


def test_helpers_on_a_hand_made_tree():
    #        0
    #      1   4
    #     2 3
    nodes = np.zeros(5, dtype=[("right", np.int32)])
    nodes["right"] = [4, 2, 0, 0, 0]
    assert Cl.depth(nodes) == 2
    assert [c.tolist() for c in Cl.level_census(nodes)] == [[3], [2, 1], [1, 1]]
    assert Cl.depth(nodes[2:3]) == 0


@pytest.mark.parametrize("u", [1, 1000, 1380, 1381, 1382])
def test_dups_has_one_leaf_per_position(trees, u):
    c = Cl.dups(u)
    assert c.pts.shape == (4000, 3) and np.unique(c.pts, axis=0).shape[0] == u
    nodes, nl = trees(c)
    assert nl == u
    if u > 1:
        assert Cl.depth(nodes) == 13
    # scenario 3: dups(1000) -> dups(u) is similar, and the three u sit one below, at and one above the pre-sized block
    assert Cl.similar(4000, 4000)
    assert [v - Cl.leaf_cap(4000, 1000) for v in Cl.DUPS_EDGE] == [-1, 0, 1]


def test_blob_tail_depths_and_leaf_counts(trees):
    got = {k: trees(Cl.blob_tail(k)) for k in Cl.TAILS_B}
    assert {k: Cl.depth(got[k][0]) for k in Cl.TAILS_B} == Cl.BLOB_DEPTH
    assert [Cl.BLOB_DEPTH[k] for k in Cl.TAILS_A] == [14, 16, 17, 18]
    leaves = {k: got[k][1] for k in Cl.TAILS_B}
    assert all(3500 <= v <= 3560 for v in leaves.values()), leaves
    # scenario 5: every B fits the block sized from every A, so that only the depth decides about the pre-sized tree
    for a in Cl.TAILS_A:
        for b in Cl.TAILS_B:
            assert leaves[b] <= Cl.leaf_cap(4000, leaves[a])
    # ... and the pairs cover: no extra round, one, two (eight steps each behind the first 18 .. 20)
    rounds = {(a, b): max(0, -(-(Cl.BLOB_DEPTH[b] + 1 - Cl.first_steps(Cl.BLOB_DEPTH[a])) // 8)) for a in Cl.TAILS_A for b in Cl.TAILS_B}
    assert set(rounds.values()) == {0, 1, 2}
    # scenario 4 / 9: the records checks need 1 000 leaves
    assert min(leaves.values()) >= 1000


def test_blob_heads_either_side_of_similar(trees):
    assert np.array_equal(Cl.blob_head(4000).pts, Cl.blob_tail(0).pts)
    for n in Cl.HEADS:
        c = Cl.blob_head(n)
        assert c.pts.shape == (n, 3)
        assert trees(c)[1] >= 1000
    one = Cl.blob_head(95, 1e3)
    nodes, nl = trees(one)
    assert nl == 1 and Cl.depth(nodes) == 0 and Cl.similar(95, 95)
    nodes, nl = trees(Cl.blob_head(141))
    assert Cl.similar(141, 141) and nl > 1


def test_gauss40k_census(trees):
    nodes, nl = trees(Cl.gauss40k(1e3))
    assert nl == 1 and Cl.depth(nodes) == 0
    nodes, nl = trees(Cl.gauss40k(1e-5))
    assert nl == 40000 and Cl.depth(nodes) == 18
    cen = Cl.level_census(nodes)  # (every point a leaf: leaves under a node == its points)
    l6, l7 = cen[6], cen[7]
    assert l6.size == 64 and int((l6 > 512).sum()) == 42 and int(((l6 > 32) & (l6 <= 512)).sum()) == 22
    assert l7.size == 128 and int(((l7 > 32) & (l7 <= 512)).sum()) == 128
    # scenario 1: behind the one-leaf tree every step is launched with 24 workgroups (need 0): 42 team nodes on 23 of them
    assert Cl.similar(40000, 40000) and Cl.leaf_cap(40000, 1) < nl and int((l6 > 512).sum()) > 23
    assert Cl.first_steps(0) == 18 <= Cl.depth(nodes)


def test_line2_depths(trees):
    for (lo, hi), want in ((Cl.LINE_DEEP, 94), ((-48, 47), Cl.MAX_DEPTH), ((-48, 48), Cl.MAX_DEPTH + 1), (Cl.LINE_REFUSED, 120)):
        c = Cl.line2(lo, hi)
        nodes, nl = trees(c)
        assert Cl.depth(nodes) == want, (lo, hi)
        if want <= 96:  # one point peeled per level
            assert c.pts.shape[0] == want + 1 == nl
            assert all(sorted(lv.tolist()) == [1, nl - l] for l, lv in enumerate(Cl.level_census(nodes)) if l > 0)
    assert Cl.LINE_REFUSED[1] - Cl.LINE_REFUSED[0] + 1 == 141
