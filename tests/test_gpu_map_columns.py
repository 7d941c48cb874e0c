"""Every column a device map can have survives everything that moves rows (mad_icp_amd/csrc/common/map_layout.h has the list;
frontend_capi.inc.h loops over it at a growth, in the removal log and in the downloads, and hands fe::map_compact /
fe::map_log_removed the columns as two structs).  For each of the eight combinations of (attribute, evidence, moments) a device map
made for ONE row and its host twin run the same short script — three folds, which grow the block at least three times, a prune of
about half the rows, another fold, a clearing, the log — and after every step every column the map has, and at the end the log, is
bit-equal to the twin's: rows, stored keys, words, evidence, the ten moment words.  One more case on the map with every column has
exactly 4 097 rows in front of the prune.  A column dropped from one of the loops fails here by name."""
import numpy as np
import pytest

from map_impls import maps  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

VOXEL = 0.5
EVIDENCE = (2, 1, 6)  # hit, miss, cap
MAX_COUNT = 1000
R, T = np.eye(3), np.array([0.125, -0.25, 0.0625])
PRUNE_RADIUS = 3.9  # the sphere of half a cube of side 8: (4 / 3) pi r^3 = 256
COMBOS = [(a, e, m) for m in (False, True) for e in (False, True) for a in (False, True)]


def random_clouds():
    """four clouds of 300 points in a cube of side 8 about the origin — 4 096 voxels: most points open one, some fall into an older
    one — each with a word per point"""
    rng = np.random.default_rng(20)
    return [(rng.uniform(-4.0, 4.0, (300, 3)), rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)) for _ in range(4)]


def lattice_clouds():
    """three clouds that open 4 097 voxels between them (one point at the centre of each, a few twice) and a fourth beside them"""
    i = np.arange(4097 + 300)
    xyz = (np.stack([i % 17, (i // 17) % 17, i // 289], axis=1) + 0.5) * VOXEL - np.array([4.0, 4.0, 4.0]) - T
    words = (i * 2654435761 % (1 << 32)).astype(np.uint32)
    cuts = [(0, 1366), (1300, 2732), (2700, 4097), (4097, 4397)]
    return [(xyz[a:b].copy(), words[a:b].copy()) for a, b in cuts]


def spec(attr, ev, mom):
    """a map made for ONE row with these columns and the removal log, as the adapters of tests/map_impls.py take it"""
    return dict(voxel=VOXEL, initial_rows=1, max_rows=1 << 20, with_attr=attr, evidence=EVIDENCE if ev else None,
                max_count=MAX_COUNT if mom else None, tracking=True)


def log(m):
    return dict(zip(("keys", "xyz", "attr"), m.take()))


def same(step, got, want):
    assert sorted(got) == sorted(want), step
    for name in want:
        assert got[name].shape == want[name].shape, (step, name, got[name].shape, want[name].shape)
        assert got[name].tobytes() == want[name].tobytes(), (step, name)


def run_script(dev, twin, clouds, rows_before_prune=None):
    def both(step, call):
        got, want = call(dev), call(twin)
        assert got == want, (step, got, want)
        same(step, dev.columns(), twin.columns())
        return want

    cap, growths = 1, 0  # (madicp_hip.h's growth rule: a fold of n points into M rows of a block for fewer than M + n grows it)
    for k in range(3):
        need = twin.size() + clouds[k][0].shape[0]
        if need > cap:
            cap, growths = max(need, 2 * cap), growths + 1
        both("fold %d" % k, lambda m: m.insert(clouds[k][0], R, T, clouds[k][1], key=k))
    assert growths >= 3
    rows = twin.size()
    if rows_before_prune is not None:
        assert rows == rows_before_prune
    removed, kept, _ = both("prune", lambda m: m.prune((0.0, 0.0, 0.0), PRUNE_RADIUS, rows))
    assert 0.3 * rows < removed < 0.7 * rows, (removed, rows)
    both("fold behind the prune", lambda m: m.insert(clouds[3][0], R, T, clouds[3][1], key=3))
    removed, _, _ = both("clearing", lambda m: m.clear_rays(clouds[1][0], R, T, wm=twin.size(), words=clouds[1][1], key=1))
    assert removed > 0 or dev.params is not None
    got, want = log(dev), log(twin)
    assert want["keys"].shape[0] > 0
    same("the log", got, want)
    same("behind the take", dev.columns(), twin.columns())


@pytest.fixture
def pair(ctx, maps):
    """a device map, whose scans always get their words and stay resident per key, and its host twin, whose folds always go through
    madicp_host_map_insert_attr"""
    return lambda attr, ev, mom: (maps.dev(ctx, set_attr=True, **spec(attr, ev, mom)), maps.host(insert_attr=True, **spec(attr, ev, mom)))


@pytest.mark.parametrize("attr,ev,mom", COMBOS)
def test_every_column_follows_its_rows(pair, attr, ev, mom):
    dev, twin = pair(attr, ev, mom)
    run_script(dev, twin, random_clouds())


def test_one_row_over_the_scan_tile(pair):
    """4 097 rows in front of the prune, on the map with every column"""
    dev, twin = pair(True, True, True)
    run_script(dev, twin, lattice_clouds(), rows_before_prune=4097)
