"""Clouds that make one hint of the device tree builder wrong, and the preconditions of that as code.

TEST INFRASTRUCTURE ONLY (no GPU).  The device builder sizes the launches of a build from what the same context built last
(frontend_capi.inc.h, tree_build_begin_on: FrontScratch::last_n / last_depth / last_leaves / last_need).  Every cloud here is
seeded, and chosen so that built after another one of this file a specific hint is wrong: the depth, the leaf count, the work
per step, or the similarity of the two point counts.  tests/test_tree_history_clouds.py holds every property claimed below
with the HOST builder, so that tests/test_gpu_tree_build_history.py cannot pass by missing the branch it is aimed at.

  dups(u)          u distinct positions, 4 000 points drawn from them, b_max 1e-5: exactly u leaves
  blob_tail(k)     a flat 4 000-point Gaussian blob whose last k points lie a factor 100 apart on the x axis: every tail
                   point costs one level, the leaf count hardly moves
  gauss40k(b_max)  40 000 points: one leaf at b_max 1e3; 40 000 leaves at 1e-5, with more team-regime nodes (> 512 points) on
                   level 6 than the cropped launch has workgroups
  line2(lo, hi)    the points 100^i on the x axis: every split peels one point, depth == n - 1
"""
import collections
import functools

import numpy as np

import descent_ref as D

B_MIN = 0.1
Cloud = collections.namedtuple("Cloud", "name pts b_max b_min")

BLOB_SCALE = (6.0, 2.5, 0.4)
BLOB_SEED = 0       # the seed at which blob_tail(k) has the depths of BLOB_DEPTH (test_tree_history_clouds.py holds it)
GAUSS_SEED = 6      # ... and gauss40k 42 team-regime nodes on level 6 (seeds 0 .. 5 give 40 .. 43)
DUPS_SEED = 1       # ... and dups(u) is 13 levels deep for u = 1000, 1380, 1381, 1382
BLOB_DEPTH = {0: 14, 4: 16, 6: 17, 8: 18, 10: 19, 12: 20, 16: 22, 20: 24, 30: 29}  # tail points -> depth of the host tree


def _frozen(name, pts, b_max, b_min=B_MIN):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    pts.setflags(write=False)
    return Cloud(name, pts, float(b_max), float(b_min))


@functools.lru_cache(maxsize=None)
def dups(u, n=4000):
    """`u` distinct uniform positions in [-20, 20]^3 and `n` points drawn from them: each position at least once, shuffled.
    A node of one position has extent 0 and is a leaf, a node of two is 1e-5 wide with probability 0: u leaves."""
    rng = np.random.default_rng([DUPS_SEED, u])
    pos = rng.uniform(-20.0, 20.0, size=(u, 3))
    pick = np.concatenate([np.arange(u), rng.integers(0, u, size=n - u)])
    rng.shuffle(pick)
    return _frozen("dups(%d)" % u, pos[pick], 1e-5)


@functools.lru_cache(maxsize=None)
def blob(n, seed=BLOB_SEED):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 3)) * BLOB_SCALE
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def blob_tail(k, n=4000):
    """The blob with its last k points replaced by (1e3 * 100^i, 0, 0), i < k."""
    a = blob(n).copy()
    if k:
        a[n - k:] = 0.0
        a[n - k:, 0] = 1e3 * 100.0 ** np.arange(k)
    return _frozen("blob_tail(%d)" % k, a, 0.2)


@functools.lru_cache(maxsize=None)
def blob_head(n, b_max=0.2, of=4600):
    """The first n points of an `of`-point blob (the clouds either side of `similar`; at b_max 1e3 a one-leaf tree)."""
    return _frozen("blob_head(%d, %g, %d)" % (n, b_max, of), blob(of)[:n], b_max)


@functools.lru_cache(maxsize=None)
def gauss40k(b_max):
    rng = np.random.default_rng(GAUSS_SEED)
    return _frozen("gauss40k(%g)" % b_max, rng.normal(size=(40000, 3)) * BLOB_SCALE, b_max)


@functools.lru_cache(maxsize=None)
def line2(lo, hi):
    """(100^i, 0, 0), i = lo .. hi.  Both signs of the exponent: a one-sided line stops near 76 levels, where 100^(2k) overflows."""
    x = 100.0 ** np.arange(lo, hi + 1, dtype=np.float64)
    return _frozen("line2(%d, %d)" % (lo, hi), np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1), 100.0 ** lo * 1e-6, 1e-160)


# ---- over a host tree's `right` links ------------------------------------------------------------------------------------
def depth(nodes):
    """The deepest level of the preorder array (a single leaf: 0)."""
    return int(D.levels(nodes).max())


def level_census(nodes):
    """-> list over the levels: the number of leaves under every node of that level, in preorder."""
    lev = D.levels(nodes)
    leaves = (D.subtree_sizes(nodes) + 1) // 2
    return [leaves[lev == l] for l in range(int(lev.max()) + 1)]


# ---- the builder's two integer rules (tree_build_begin_on) ------------------------------------------------------------------
def similar(n, last_n):
    """Whether a build of n points takes the hints of a build of last_n points."""
    return last_n > 0 and last_n - last_n // 8 <= n <= last_n + last_n // 8


def leaf_cap(n, last_leaves):
    """Leaves the block of the pre-sized emission has room for."""
    return min(n, last_leaves + last_leaves // 8 + 256)


def first_steps(last_depth):
    """Steps a build launches before it looks, behind a similar build `last_depth` levels deep (-1: no hint)."""
    return 20 if last_depth < 0 else min(20, max(last_depth + 2, 18))


def host_tree(cloud):
    from mad_icp_amd import capi

    return capi.HostTree(cloud.pts, cloud.b_max, cloud.b_min, 2)


# ---- what the scenarios of tests/test_gpu_tree_build_history.py are made of --------------------------------------------------
DUPS_EDGE = (1380, 1381, 1382)           # behind dups(1000): one below, at, one above leaf_cap(4000, 1000) == 1381
TAILS_A = (0, 4, 6, 8)                   # blob_tail(k) built first: 18, 18, 19, 20 steps for the build behind it
TAILS_B = (0, 4, 6, 8, 10, 12, 16, 20, 30)
HEADS = (3499, 3500, 4500, 4501)         # point counts either side of similar(n, 4000)
LINE_DEEP = (-47, 47)                    # depth 94: the deepest rounds of the continue-and-check loop
LINE_REFUSED = (-70, 70)                 # depth 120
MAX_DEPTH = 95  # the deepest tree the device builds (tree_build.hip.h, kMaxLevels = 96 steps: 0 .. 95, one level each)
