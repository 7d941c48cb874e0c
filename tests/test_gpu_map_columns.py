"""Every column a device map can have survives everything that moves rows (mad_icp_amd/csrc/common/map_layout.h has the list;
frontend_capi.inc.h loops over it at a growth, in the removal log and in the downloads, and hands fe::map_compact /
fe::map_log_removed the columns as two structs).  For each of the eight combinations of (attribute, evidence, moments) a device map
made for ONE row and its host twin run the same short script — three folds, which grow the block at least three times, a prune of
about half the rows, another fold, a clearing, the log — and after every step every column the map has, and at the end the log, is
bit-equal to the twin's: rows, stored keys, words, evidence, the ten moment words.  One more case on the map with every column has
exactly 4 097 rows in front of the prune.  A column dropped from one of the loops fails here by name."""
import numpy as np
import pytest

from mad_icp_amd import capi

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


class DevMap:
    def __init__(self, ctx, attr, ev, mom):
        self.ctx, self.attr, self.ev, self.mom = ctx, attr, ev, mom
        if mom:
            self.mid = ctx.map_create_mom(VOXEL, 1, 1 << 20, MAX_COUNT, with_attr=attr, evidence=EVIDENCE if ev else None)
        elif ev:
            self.mid = ctx.map_create_ev(VOXEL, 1, 1 << 20, *EVIDENCE, with_attr=attr)
        else:
            self.mid = ctx.map_create_attr(VOXEL, 1, 1 << 20) if attr else ctx.map_create(VOXEL, 1, 1 << 20)
        ctx.map_track_removed(self.mid, True)
        self.clouds = {}

    def cloud(self, k, xyz, words):
        if k not in self.clouds:
            self.clouds[k] = self.ctx.cloud_upload(xyz)
            self.ctx.cloud_set_attr(self.clouds[k], words)
        return self.clouds[k]

    def fold(self, k, xyz, words):
        return self.ctx.map_insert_cloud(self.mid, self.cloud(k, xyz, words), R, T)

    def prune(self, radius, watermark):
        return self.ctx.map_prune(self.mid, (0.0, 0.0, 0.0), radius, watermark)

    def clear_rays(self, k, xyz, words, watermark):
        return self.ctx.map_clear_rays(self.mid, self.cloud(k, xyz, words), R, T, watermark=watermark)

    def size(self):
        return self.ctx.map_size(self.mid)

    def columns(self):
        got = dict(zip(("xyz", "keys", "attr"), self.ctx.map_download_rows(self.mid, with_keys=True, with_attr=self.attr)))
        if self.ev:
            got["evidence"] = self.ctx.map_download_evidence(self.mid)
        if self.mom:
            got["moments"] = self.ctx.map_download_moments(self.mid)
        return got

    def take(self):
        return dict(zip(("keys", "xyz", "attr"), self.ctx.map_take_removed(self.mid, with_attr=self.attr)))

    def close(self):
        for cid in self.clouds.values():
            self.ctx.cloud_release(cid)
        self.ctx.map_release(self.mid)


class Twin:
    def __init__(self, attr, ev, mom):
        self.attr, self.ev, self.mom = attr, ev, mom
        if mom:
            self.h = capi.host_map_create_mom(VOXEL, 1, 1 << 20, MAX_COUNT, with_attr=attr, evidence=EVIDENCE if ev else None)
        elif ev:
            self.h = capi.host_map_create_ev(VOXEL, 1, 1 << 20, *EVIDENCE, with_attr=attr)
        else:
            self.h = capi.host_map_create_attr(VOXEL, 1, 1 << 20) if attr else capi.host_map_create(VOXEL, 1, 1 << 20)
        capi.host_map_track_removed(self.h, True)

    def fold(self, k, xyz, words):
        return capi.host_map_insert_attr(self.h, xyz, words, R, T)

    def prune(self, radius, watermark):
        return capi.host_map_prune(self.h, (0.0, 0.0, 0.0), radius, watermark)

    def clear_rays(self, k, xyz, words, watermark):
        return capi.host_map_clear_rays(self.h, xyz, R, T, watermark=watermark)

    def size(self):
        return capi.host_map_size(self.h)

    def columns(self):
        got = dict(zip(("xyz", "keys", "attr"), capi.host_map_download_rows(self.h, with_keys=True, with_attr=self.attr)))
        if self.ev:
            got["evidence"] = capi.host_map_download_evidence(self.h)
        if self.mom:
            got["moments"] = capi.host_map_download_moments(self.h)
        return got

    def take(self):
        return dict(zip(("keys", "xyz", "attr"), capi.host_map_take_removed(self.h, with_attr=self.attr)))

    def close(self):
        capi.host_map_destroy(self.h)


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
        both("fold %d" % k, lambda m: m.fold(k, *clouds[k]))
    assert growths >= 3
    rows = twin.size()
    if rows_before_prune is not None:
        assert rows == rows_before_prune
    removed, kept, _ = both("prune", lambda m: m.prune(PRUNE_RADIUS, rows))
    assert 0.3 * rows < removed < 0.7 * rows, (removed, rows)
    both("fold behind the prune", lambda m: m.fold(3, *clouds[3]))
    removed, _, _ = both("clearing", lambda m: m.clear_rays(1, *clouds[1], watermark=twin.size()))
    assert removed > 0 or dev.ev
    got, want = dev.take(), twin.take()
    assert want["keys"].shape[0] > 0
    same("the log", got, want)
    same("behind the take", dev.columns(), twin.columns())


@pytest.fixture
def pair(ctx):
    alive = []

    def make(attr, ev, mom):
        alive.extend([DevMap(ctx, attr, ev, mom), Twin(attr, ev, mom)])
        return alive[-2], alive[-1]

    yield make
    for m in alive:
        m.close()


@pytest.mark.parametrize("attr,ev,mom", COMBOS)
def test_every_column_follows_its_rows(pair, attr, ev, mom):
    dev, twin = pair(attr, ev, mom)
    run_script(dev, twin, random_clouds())


def test_one_row_over_the_scan_tile(pair):
    """4 097 rows in front of the prune, on the map with every column"""
    dev, twin = pair(True, True, True)
    run_script(dev, twin, lattice_clouds(), rows_before_prune=4097)
