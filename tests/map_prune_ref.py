"""Map + prune (include/madicp_hip.h: madicp_map_insert_cloud, madicp_map_prune) restated in numpy with a Python set, and the
sequences the host and the device tests share.  The fold is voxel_map_ref.RefMap's rule, restated here because a prune needs every
row's KEY (from the float64 position — a float row cannot reproduce it) and its attribute word, which RefMap does not keep.
The prune, everything in float64 from the STORED float32 row:
  d2     = dx*dx + (dy*dy + dz*dz),  dx = float64(row[0]) - center[0] ...
  kept   d2 <= radius*radius (exactly radius: kept; NaN: removed); kept rows close up in order, keys and words with them
  K      loses the keys of the removed rows
  answer (rows removed, rows left, kept rows among rows [0, watermark))"""
import numpy as np

import cloud_export_ref as E
import voxel_map_ref as V


class RefPruneMap:
    def __init__(self, voxel, max_rows=1 << 30):
        self.voxel = float(voxel)
        self.max_rows = int(max_rows)
        self.keys = set()
        self.xyz = np.empty((0, 3), np.float32)
        self.row_keys = np.empty(0, np.int64)
        self.words = np.empty(0, np.uint32)

    @property
    def size(self):
        return self.xyz.shape[0]

    def insert(self, cloud, R, t, attr=None):
        """Returns the rows added; None (map unchanged) where the real thing refuses for capacity."""
        q = E.positions(cloud, R, t)
        n = q.shape[0]
        if self.size + n > self.max_rows:
            return None
        with np.errstate(all="ignore"):
            f = np.floor(q / self.voxel)
            cand = np.all((f >= -E.CELL) & (f < E.CELL), axis=1)
        idx = np.nonzero(cand)[0]
        kept, kept_keys = [], []
        if idx.size:
            k = f[idx].astype(np.int64) + int(E.CELL)
            key = k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)
            for i, kk in zip(idx.tolist(), key.tolist()):  # ascending index: the first arrival of a key is its lowest index
                if kk not in self.keys:
                    self.keys.add(kk)
                    kept.append(i)
                    kept_keys.append(kk)
        with np.errstate(all="ignore"):
            self.xyz = np.concatenate([self.xyz, q[kept].astype(np.float32).reshape(-1, 3)], axis=0)
        self.row_keys = np.concatenate([self.row_keys, np.array(kept_keys, np.int64)])
        w = np.zeros(n, np.uint32) if attr is None else np.asarray(attr, np.uint32)
        self.words = np.concatenate([self.words, w[kept]])
        return len(kept)

    def kept_mask(self, center, radius):
        c = np.asarray(center, np.float64).reshape(3)
        r = self.xyz.astype(np.float64)
        with np.errstate(all="ignore"):
            dx, dy, dz = r[:, 0] - c[0], r[:, 1] - c[1], r[:, 2] - c[2]
            return dx * dx + (dy * dy + dz * dz) <= np.float64(radius) * np.float64(radius)

    def prune(self, center, radius, watermark=0):
        keep = self.kept_mask(center, radius)
        assert 0 <= watermark <= self.size
        before = self.size
        mark = int(np.count_nonzero(keep[:watermark]))
        for kk in self.row_keys[~keep].tolist():
            self.keys.remove(kk)
        self.xyz, self.row_keys, self.words = self.xyz[keep], self.row_keys[keep], self.words[keep]
        return before - self.size, self.size, mark

    def rows(self, first_row=0):
        return np.ascontiguousarray(self.xyz[first_row:])

    def attr(self, first_row=0):
        return np.ascontiguousarray(self.words[first_row:])

    def clear(self):
        self.__init__(self.voxel, self.max_rows)


# ---- the shared sequences: lists of steps, ("fold", points, R, t) and ("prune", center, radius, watermark) -------------------------
# watermark: an int, or a fraction of the rows the map holds at that step ("all" = every row)
VOXEL = V.VOXEL
SIZES = V.SIZES
MODES = ["none", "all", "alternate", "median"]
FRACTIONAL = np.array([0.3125, -1.7, 2.0 / 3.0])


def shells(n):
    """n points alternating between a shell of radius 30 (even index) and one of radius 90 (odd), on a spiral that keeps every
    point in a voxel of its own at voxel 0.5 (the sequences assert it: rows == n)"""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    return d * np.where(i % 2 == 0, 30.0, 90.0)[:, None]


def size_case(n, mode):
    """one cloud that gives n rows, a prune of the given kind, the cloud again (the removed voxels are new again), a second
    identical prune"""
    R, t = E.IDENTITY
    if mode == "none":
        pts, c, r, wm = E.own_cells(n), np.array([20.0, 20.0, 3.0]), 1.0e6, "all"
    elif mode == "all":
        pts, c, r, wm = E.own_cells(n), np.array([1.0e4, 0.0, 0.0]), 1.0, 0
    elif mode == "alternate":
        pts, c, r, wm = shells(n), np.zeros(3), 60.0, 0.5
    else:
        pts = E.own_cells(n) + np.random.default_rng(n).uniform(0.0, 0.4, size=(n, 3))
        c = FRACTIONAL + np.array([20.0, 20.0, 2.0])
        d = np.linalg.norm(pts.astype(np.float32).astype(np.float64) - c, axis=1)
        r, wm = float(np.median(d)), 1.0 / 3.0
    return [("fold", pts, R, t), ("prune", c, r, wm), ("fold", pts, R, t), ("prune", c, r, wm)]


def boundary():
    """centre the origin, radius 5: d2 == r2 exactly stays, one float ulp beyond leaves"""
    R, t = E.IDENTITY
    up = float(np.nextafter(np.float32(5.0), np.float32(6.0)))
    # nextafter(0, 1) as float32 scaled to 2^-24, the smallest z with 9 + (16 + z*z) > 25 in float64 (z*z = 2^-48, one ulp of 16 and
    # of 25); negative, so that at voxel 0.5 it falls into cell -1 beside (3, 4, 0)'s cell 0 — and -up into cell -11 beside 5's 10
    tiny = -float(np.nextafter(np.float32(0.0), np.float32(1.0))) * 2.0 ** 125
    assert tiny == -2.0 ** -24 and np.float32(tiny) != 0 and 9.0 + (16.0 + tiny * tiny) > 25.0
    pts = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 5.0], [3.0, 4.0, tiny], [0.0, 0.0, -up], [-5.0, 0.0, 0.0], [0.0, -up, 0.0]])
    return [("fold", pts, R, t), ("prune", np.zeros(3), 5.0, 3)]


def reentry(n=1025):
    R, t = E.IDENTITY
    pts = shells(n)
    return [("fold", pts, R, t), ("prune", np.zeros(3), 60.0, "all"), ("fold", pts, R, t), ("prune", np.zeros(3), 60.0, 0.5)]


def to_empty(n=1025):
    R, t = E.random_pose(5)
    pts = E.gaussian(n, 21)
    return [("fold", pts, R, t), ("prune", np.array([500.0, 0.0, 0.0]), 2.0, 0.5), ("fold", pts, R, t)]


def posed(n=4097):
    """a centre with a fractional part and a random pose's translation"""
    out = []
    for f in range(3):
        R, t = E.random_pose(80 + f)
        out += [("fold", E.gaussian(n, 700 + f, scale=7.0), R, t), ("prune", t + FRACTIONAL * (f % 2), 9.0, 0.5)]
    return out


def growth(frames=6, n=4097):
    """folds and prunes interleaved over frames that make a map of initial_rows = 1 grow several times"""
    out = []
    for f in range(frames):
        R, t = E.random_pose(60 + f)
        out.append(("fold", E.gaussian(n, 300 + f, scale=6.0 + f), R, t))
        if f % 2 == 1 or f == frames - 1:
            out.append(("prune", t, 9.0 + f, 0.5))
    return out


def large(clouds=80, n=256):
    """a map much larger than any cloud: 80 clouds of 256 points in distinct cells (20 480 rows), everything beyond a sphere through
    the middle of the lattice pruned out, one more cloud of new cells, and one of the first clouds again (partly new again)"""
    R, _ = E.IDENTITY
    allpts = E.own_cells(clouds * n)
    out = [("fold", allpts[k * n:(k + 1) * n], R, np.zeros(3)) for k in range(clouds)]
    c = np.array([27.0, 27.0, 11.0])
    out.append(("prune", c, 24.0, 0.5))
    out.append(("fold", allpts[:n] + np.array([0.0, 0.0, 40.0]), R, np.zeros(3)))
    out.append(("fold", allpts[5 * n:6 * n], R, np.zeros(3)))
    return out


def named(name):
    if name.startswith("size-"):
        _, n, mode = name.split("-")
        return size_case(int(n), mode)
    return {"boundary": boundary, "reentry": reentry, "to_empty": to_empty, "posed": posed, "growth": growth, "large": large}[name]()


SIZE_NAMES = ["size-%d-%s" % (n, mode) for n in SIZES for mode in MODES]
OTHER_NAMES = ["boundary", "reentry", "to_empty", "posed", "growth"]

_cache = {}


def expected(name, voxel=VOXEL):
    """the restatement run over named(name), computed once: (steps, [(answer, rows, words)]) — the fold's points carry their index
    as attribute word; a watermark given as a fraction is resolved against the restatement's rows (the step handed on has the int)"""
    k = (name, voxel)
    if k not in _cache:
        ref, steps, out = RefPruneMap(voxel), [], []
        for step in named(name):
            if step[0] == "fold":
                _, pts, R, t = step
                added = ref.insert(pts, R, t, np.arange(pts.shape[0], dtype=np.uint32))
                ans = (added, ref.size)
            else:
                _, c, r, wm = step
                wm = ref.size if wm == "all" else (int(wm * ref.size) if isinstance(wm, float) else wm)
                step = ("prune", c, r, wm)
                ans = ref.prune(c, r, wm)
            rows, words = ref.rows(), ref.attr()
            rows.setflags(write=False)
            words.setflags(write=False)
            steps.append(step)
            out.append((ans, rows, words))
        _cache[k] = (steps, out)
    return _cache[k]


def replay(name, impl, voxel=VOXEL, also=()):
    """runs named(name) through impl — an object with insert(points, R, t, words) -> (added, rows), prune(center, radius, watermark)
    -> (removed, rows, watermark), rows(), words() (None: no column) — and holds it to the restatement after EVERY step; `also`:
    further implementations held to the same.  Returns the expectations."""
    steps, want = expected(name, voxel)
    for step, (ans, rows, words) in zip(steps, want):
        for m in (impl,) + tuple(also):
            if step[0] == "fold":
                got = m.insert(step[1], step[2], step[3], np.arange(step[1].shape[0], dtype=np.uint32))
            else:
                got = m.prune(step[1], step[2], step[3])
            assert tuple(got) == tuple(ans), (name, step[0], got, ans)
            mine = m.rows()
            assert mine.dtype == np.float32 and mine.shape == rows.shape and E.same_bits(mine, rows), (name, step[0])
            w = m.words()
            if w is not None:
                assert w.dtype == np.uint32 and w.tobytes() == words.tobytes(), (name, step[0])
    return want


class RefDrive:
    """Pipeline's side of it (csrc/host/pipeline.h: setMapAccumulation + setMapRange) restated: the fold of every frame at its pose,
    the prune policy — (b) before a fold the capacity rule would refuse, once, at the position of the frame before; (a) after a
    successful fold once the position is radius / 4 from the centre of the last prune, squared distances in float64, the first
    folded position counting as one — and the consumer's cursor handed through every prune as the watermark."""

    def __init__(self, voxel, radius=0.0, max_points=1 << 24):
        self.map = RefPruneMap(voxel, max_points)
        self.radius = float(radius)
        self.center = self.last = None
        self.made = self.overflowed = False
        self.cursor = self.removed = self.prunes = 0

    def prune(self, center, radius=None):
        removed, _, self.cursor = self.map.prune(center, self.radius if radius is None else radius, self.cursor)
        self.removed += removed
        self.prunes += 1
        return removed

    def frame(self, cloud, T, attr=None):
        """one folded frame; returns the rows the fold added (None: refused, or not attempted after an overflow)"""
        pos = np.array(np.asarray(T, np.float64)[:3, 3])
        added = None
        if not self.overflowed:
            if self.radius > 0.0 and self.made and self.last is not None and self.map.size + cloud.shape[0] > self.map.max_rows:
                self.prune(self.last)
                self.center = self.last
            self.made = True
            added = self.map.insert(cloud, np.asarray(T)[:3, :3], pos, attr)
            if added is None:
                self.overflowed = True
            elif self.radius > 0.0:
                if self.center is None:
                    self.center = pos
                else:
                    d = pos - self.center
                    step = self.radius / 4.0
                    if d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]) >= step * step:
                        self.prune(pos)
                        self.center = pos
        self.last = pos
        return added

    def new_rows(self):
        """what mapNewRows returns: (rows, words) added since the last call that are still there"""
        first, self.cursor = self.cursor, self.map.size
        return self.map.rows(first), self.map.attr(first)

    def clear(self):
        self.map.clear()
        self.overflowed = False
        self.center = None
        self.cursor = self.removed = 0
