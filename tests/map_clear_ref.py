"""Free-space clearing (include/madicp_hip.h: madicp_map_clear_rays) restated in numpy, vectorised over the rays, with Python sets
for the traversed and the occupied keys — and the sequences the host and the device tests share.  Everything in float64,
elementwise (numpy does not fuse), on top of map_prune_ref.RefPruneMap (the fold, the stored keys, the words):
  qo, q[i]  the origin and point i through (R, t): cloud_export_ref.positions
  d, L      d = q[i] - qo per axis, L = sqrt(dx*dx + (dy*dy + dz*dz))
  K         min(floor((L - margin) / voxel), 4096) if L is finite and L - margin >= voxel, else 0
  sample k  s = qo + d * f per axis, f = (k * voxel) / L, k = 1 .. K
  T, O      the candidate keys of the samples / of the end points q[i]
  a row leaves iff its stored key is in T \\ O; the kept rows close up in order, keys and words with them
  answer    (rows removed, rows left, kept rows among rows [0, watermark))"""
import numpy as np

import cloud_export_ref as E
import map_prune_ref as P

MAX_SAMPLES = 4096
VOXEL = P.VOXEL


def keys_of(q, voxel):
    """(candidate mask, int64 keys of the candidates) of positions q (m, 3)"""
    with np.errstate(all="ignore"):
        f = np.floor(q / voxel)
        cand = np.all((f >= -E.CELL) & (f < E.CELL), axis=1)
    k = f[cand].astype(np.int64) + int(E.CELL)
    return cand, k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)


def ray_sets(cloud, R, t, origin, margin, voxel):
    """(T, O): the keys the rays traverse and the keys their end points occupy"""
    q = E.positions(cloud, R, t)
    qo = E.positions(np.asarray(origin, np.float64).reshape(1, 3), R, t)[0]
    margin = np.float64(margin)
    with np.errstate(all="ignore"):
        d = q - qo
        L = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
        reach = L - margin
        walks = np.isfinite(L) & (reach >= voxel)
        K = np.zeros(q.shape[0], np.int64)
        K[walks] = np.minimum(np.floor(reach[walks] / voxel), float(MAX_SAMPLES)).astype(np.int64)
    occupied = set(keys_of(q, voxel)[1].tolist())
    traversed = set()
    for k in range(1, int(K.max(initial=0)) + 1):
        on = K >= k
        with np.errstate(all="ignore"):
            f = (np.float64(k) * voxel) / L[on]
            s = qo + d[on] * f[:, None]
        traversed.update(keys_of(s, voxel)[1].tolist())
    return traversed, occupied


class RefClearMap(P.RefPruneMap):
    def cleared_mask(self, cloud, R, t, origin=(0.0, 0.0, 0.0), margin=0.0):
        """True where a row LEAVES"""
        traversed, occupied = ray_sets(cloud, R, t, origin, margin, self.voxel)
        gone = traversed - occupied
        return np.array([k in gone for k in self.row_keys.tolist()], dtype=bool)

    def clear_rays(self, cloud, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, watermark=0):
        assert 0 <= watermark <= self.size
        keep = ~self.cleared_mask(cloud, R, t, origin, margin) if self.size else np.zeros(0, bool)
        before = self.size
        mark = int(np.count_nonzero(keep[:watermark]))
        for kk in self.row_keys[~keep].tolist():
            self.keys.remove(kk)
        self.xyz, self.row_keys, self.words = self.xyz[keep], self.row_keys[keep], self.words[keep]
        return before - self.size, self.size, mark


# ---- the shared sequences: ("fold", points, R, t) and ("clear", points, R, t, origin, margin, watermark) ---------------------------
# points are in the CLOUD's frame; watermark: an int, a fraction of the rows the map holds at that step, or "all"
RAY_SIZES = [1, 63, 64, 65, 255, 256, 257, 1025, 4097]
MAP_SIZES = [1, 255, 256, 257, 1025, 4097]
ORIGIN = np.array([-3.3125, -2.1, 0.7])


def through(points, origin, scale):
    """targets on the rays from origin through `points`, `scale` (per ray) times as far: 1.6 looks through a point's voxel, 1.0
    ends in it, 0.5 stops short"""
    return origin + (points - origin) * np.asarray(scale, np.float64).reshape(-1, 1)


def into_cloud_frame(targets, R, t):
    """the cloud whose points (R, t) takes (nearly) to `targets`"""
    return (np.asarray(targets) - t) @ R


def size_case(m, n, seed=0):
    """a map of m rows (own_cells: one voxel each), cleared by n rays from ORIGIN through randomly chosen rows — beyond them, into
    them and short of them in equal parts — under a random pose; then the map's cloud again (cleared voxels are new again), the
    same clear at another watermark, and a growth"""
    rng = np.random.default_rng(1000 * m + n + seed)
    R, t = E.random_pose(m + n)
    cells = E.own_cells(m)
    targets = through(cells[rng.integers(0, m, size=n)], ORIGIN, rng.choice([1.6, 1.0, 0.5], size=n))
    rays = into_cloud_frame(targets, R, t)
    o = into_cloud_frame(ORIGIN[None], R, t)[0]
    I, z = E.IDENTITY
    return [("fold", cells, I, z), ("clear", rays, R, t, o, 0.0, 0.5), ("fold", cells, I, z), ("clear", rays, R, t, o, 0.25, "all"),
            ("fold", E.gaussian(3 * m + 7, m, scale=30.0), R, t)]


def edges():
    """the per-ray edges, identity pose, origin 0, voxel 0.5, margin 0.25: the map is a line of voxels along +x (cells 0 .. 8), one
    along +y and -y, and far rows around the sample cap; see tests/test_host_map_clear.py for what each ray does"""
    I, z = E.IDENTITY
    line = np.array([[0.5 * c + 0.25, 0.25, 0.25] for c in range(9)])
    ys = np.array([[0.25, 0.5 * c + 0.25, 0.25] for c in range(1, 6)] + [[0.25, -0.5 * c - 0.25, 0.25] for c in range(1, 6)])
    far = np.array([[2046.75, 0.25, 0.25], [2047.25, 0.25, 0.25], [2047.75, 0.25, 0.25], [2048.25, 0.25, 0.25], [2048.75, 0.25, 0.25],
                    [3000.25, 0.25, 0.25]])
    corner = np.array([[524188.25, 524188.25, 0.25]])  # inside the key range, between an origin and an end point outside it
    out_of_range = 524288.0 + 10.0
    rays = np.array([
        [0.25, 0.25, 0.25],                           # the origin itself, L = 0: walks nothing, protects its voxel (cell 0 of the line)
        [0.25, 0.25 + np.nextafter(0.75, 0.0), 0.25],  # L just under voxel + margin: walks nothing, protects +y cell 1
        [0.25, 0.25 - 1.3, 0.25],                     # L = 1.3: two samples along -y; ends in -y cell 3
        [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [-np.inf, 0.0, 0.0],  # no length, no key: nothing walked, nothing protected
        [out_of_range, 0.25, 0.25],                   # end point outside the key range, 4096 samples inside: the cap
    ])
    return [("fold", np.concatenate([line, ys, far, corner]), I, z), ("clear", rays, I, z, np.array([0.25, 0.25, 0.25]), 0.25, 7),
            ("fold", np.concatenate([line, ys, far, corner]), I, z),
            # an origin OUTSIDE the key range: the ray cuts the range's corner — its first and last samples have no key and are
            # skipped, the walk goes on in between (a straight ray meets the convex range once: it cannot leave it and come back)
            ("clear", np.array([[523988.25, 524388.25, 0.25]]), I, z, np.array([524388.25, 523988.25, 0.25]), 0.0, 0),
            ("fold", np.concatenate([line, ys, far, corner]), I, z)]


def exact_lengths():
    """voxel 0.5, margin 0.25, rays along the axes from origins chosen so that the last sample and the end point fall into
    DIFFERENT voxels and every length is exact in float64 (tests/test_host_map_clear.py spells out what leaves):
      +x  L = 0.75 exactly = voxel + margin: ONE sample          -y  L one ulp below 0.75: none
      +z  L - margin = 2.0 exactly: FOUR samples                 -z  L - margin one ulp below 2.0: three (second clear), and
                                                                     exactly 2.0 again (third clear): four"""
    I, z = E.IDENTITY
    rows = np.array([[0.5 * c + 0.25, 0.25, 0.25] for c in range(1, 4)] + [[0.25, -0.5 * c + 0.25, 0.25] for c in range(1, 4)] +
                    [[0.25, 0.25, 0.5 * c + 0.25] for c in range(1, 7)] + [[0.25, 0.25, -0.5 * c + 0.25] for c in range(1, 7)])
    o1, o2 = np.array([0.375, 0.125, 0.375]), np.array([0.375, 0.125, 0.125])
    rays1 = np.array([o1 + [0.75, 0.0, 0.0], o1 - [0.0, np.nextafter(0.75, 0.0), 0.0], o1 + [0.0, 0.0, 2.25]])
    under, exact = np.array([o2 - [0.0, 0.0, np.nextafter(2.25, 0.0)]]), np.array([o2 - [0.0, 0.0, 2.25]])
    return [("fold", rows, I, z), ("clear", rays1, I, z, o1, 0.25, "all"), ("fold", rows, I, z), ("clear", under, I, z, o2, 0.25, 0),
            ("fold", rows, I, z), ("clear", exact, I, z, o2, 0.25, 0), ("fold", rows, I, z)]


def protected():
    """a voxel one ray traverses and another ends in stays; so does a voxel that one ray both traverses (its last sample) and ends
    in (margin 0); the voxels in front of them leave"""
    I, z = E.IDENTITY
    rows = np.array([[0.5 * c + 0.25, 0.25, 0.25] for c in range(1, 9)] + [[0.25, 0.5 * c + 0.25, 0.25] for c in range(1, 6)])
    rays = np.array([[4.3, 0.25, 0.25], [2.3, 0.3, 0.2], [0.25, 2.6, 0.25]])
    return [("fold", rows, I, z), ("clear", rays, I, z, np.array([0.25, 0.25, 0.25]), 0.0, 4), ("fold", rows, I, z)]


def contended(n=4097):
    """all rays through ONE voxel (and on to scattered end points): one flag word for the whole launch"""
    I, z = E.IDENTITY
    rng = np.random.default_rng(5)
    eye = np.array([10.25, 10.25, 5.25])
    rows = np.concatenate([eye[None], E.own_cells(300) + np.array([0.0, 0.0, 30.0])])
    pin = eye + rng.uniform(-0.2, 0.2, size=(n, 3))
    return [("fold", rows, I, z), ("clear", through(pin, ORIGIN, rng.uniform(1.5, 3.0, size=n)), I, z, ORIGIN, 0.0, 1), ("fold", rows, I, z)]


def nothing(n=1025):
    """the folded cloud itself at its own pose: every row's voxel holds a point of the scan — nothing leaves"""
    R, t = E.random_pose(9)
    pts = E.gaussian(n, 31)
    return [("fold", pts, R, t), ("clear", pts, R, t, np.zeros(3), 0.0, 0.5), ("fold", E.gaussian(n, 32), R, t)]


def but_the_endpoints(m=1025):
    """rows in front of a scan and the scan's own rows: the first leave, the second stay"""
    I, z = E.IDENTITY
    cells = E.own_cells(m) + np.array([0.0, 0.0, 3.0])
    beyond = through(cells, ORIGIN, np.full(m, 1.7))
    return [("fold", cells, I, z), ("fold", beyond, I, z), ("clear", beyond, I, z, ORIGIN, 0.0, 0.5), ("fold", cells, I, z)]


def everything(m=1025):
    """every row is seen through: the map is empty afterwards; the cloud again is a first fold, then a growth"""
    R, t = E.random_pose(4)
    cells = E.own_cells(m) + np.array([0.0, 0.0, 3.0])
    rays = into_cloud_frame(through(cells, ORIGIN, np.full(m, 1.7)), R, t)
    o = into_cloud_frame(ORIGIN[None], R, t)[0]
    I, z = E.IDENTITY
    return [("fold", cells, I, z), ("clear", rays, R, t, o, 0.0, 0.5), ("fold", cells, I, z), ("fold", E.gaussian(5000, 8, scale=40.0), R, t)]


def large(clouds=80, n=256):
    """a map much larger than any cloud: 80 clouds of 256 points in distinct cells (20 480 rows), cleared by 256 rays"""
    I, z = E.IDENTITY
    allpts = E.own_cells(clouds * n)
    out = [("fold", allpts[k * n:(k + 1) * n], I, z) for k in range(clouds)]
    rays = through(allpts[37::80], ORIGIN, np.full(n, 1.3))
    out.append(("clear", rays, I, z, ORIGIN, 0.0, 0.5))
    out.append(("fold", allpts[5 * n:6 * n], I, z))
    return out


def scene():
    """what the feature is for.  Frame 1: a wall at x = 10 with a box in front of it (x = 6); frame 2: the same rays with the box
    gone — every ray reaches the wall.  (steps, the box's bounds)"""
    I, z = E.IDENTITY
    az, el = np.meshgrid(np.deg2rad(np.linspace(-30.0, 30.0, 121)), np.deg2rad(np.linspace(-10.0, 10.0, 17)))
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1).reshape(-1, 3)
    wall = d * (10.0 / d[:, 0])[:, None]
    at_box = d * (6.0 / d[:, 0])[:, None]
    hits_box = (np.abs(at_box[:, 1]) < 1.0) & (np.abs(at_box[:, 2]) < 0.6)
    frame1 = np.where(hits_box[:, None], at_box, wall)
    return [("fold", frame1, I, z), ("fold", wall, I, z), ("clear", wall, I, z, np.zeros(3), 0.0, 0)], hits_box, frame1, wall


def named(name):
    if name.startswith("size-"):
        _, m, n = name.split("-")
        return size_case(int(m), int(n))
    if name == "scene":
        return scene()[0]
    return {"edges": edges, "exact_lengths": exact_lengths, "protected": protected, "contended": contended, "nothing": nothing,
            "but_the_endpoints": but_the_endpoints, "everything": everything, "large": large}[name]()


SIZE_NAMES = ["size-1025-%d" % n for n in RAY_SIZES] + ["size-%d-257" % m for m in MAP_SIZES]
OTHER_NAMES = ["edges", "exact_lengths", "protected", "contended", "nothing", "but_the_endpoints", "everything", "scene"]

_cache = {}


def expected(name, voxel=VOXEL):
    """the restatement run over named(name), computed once: (steps, [(answer, rows, words)]) — a fold's points carry their index as
    attribute word; a watermark given as a fraction is resolved against the restatement's rows (the step handed on has the int)"""
    k = (name, voxel)
    if k not in _cache:
        ref, steps, out = RefClearMap(voxel), [], []
        for step in named(name):
            if step[0] == "fold":
                _, pts, R, t = step
                ans = (ref.insert(pts, R, t, np.arange(pts.shape[0], dtype=np.uint32)), ref.size)
            else:
                _, pts, R, t, o, margin, wm = step
                wm = ref.size if wm == "all" else (int(wm * ref.size) if isinstance(wm, float) else wm)
                step = ("clear", pts, R, t, o, margin, wm)
                ans = ref.clear_rays(pts, R, t, o, margin, wm)
            rows, words = ref.rows(), ref.attr()
            rows.setflags(write=False)
            words.setflags(write=False)
            steps.append(step)
            out.append((ans, rows, words))
        _cache[k] = (steps, out)
    return _cache[k]


def replay(name, impl, voxel=VOXEL, also=()):
    """runs named(name) through impl — insert(points, R, t, words) -> (added, rows), clear_rays(points, R, t, origin, margin,
    watermark) -> (removed, rows, watermark), rows(), words() (None: no column) — and holds it to the restatement after EVERY step
    (the fold behind a clear holds the stored KEYS to it: a key wrongly kept or dropped changes what is new); `also`: further
    implementations held to the same.  Returns the expectations."""
    steps, want = expected(name, voxel)
    for i, (step, (ans, rows, words)) in enumerate(zip(steps, want)):
        for m in (impl,) + tuple(also):
            if step[0] == "fold":
                got = m.insert(step[1], step[2], step[3], np.arange(step[1].shape[0], dtype=np.uint32))
            else:
                got = m.clear_rays(*step[1:])
            assert tuple(got) == tuple(ans), (name, i, step[0], got, ans)
            mine = m.rows()
            assert mine.dtype == np.float32 and mine.shape == rows.shape and E.same_bits(mine, rows), (name, i, step[0])
            w = m.words()
            if w is not None:
                assert w.dtype == np.uint32 and w.tobytes() == words.tobytes(), (name, i, step[0])
    return want


class RefDrive(P.RefDrive):
    """Pipeline's side of it (csrc/host/pipeline.h: setMapAccumulation + setMapClearing + setMapRange) restated: the fold of every
    frame at its pose, the clearing by the cloud just folded with the consumer's cursor as the watermark, then the range prune."""

    def __init__(self, voxel, radius=0.0, max_points=1 << 24, clearing=True, margin=0.0, origin=(0.0, 0.0, 0.0)):
        super().__init__(voxel, radius, max_points)
        self.map = RefClearMap(voxel, max_points)
        self.clearing, self.margin, self.origin = clearing, margin, np.asarray(origin, np.float64)
        self.cleared = 0

    def clear_rays(self, cloud, T, origin=None, margin=None):
        T = np.asarray(T, np.float64)
        removed, _, self.cursor = self.map.clear_rays(cloud, T[:3, :3], np.array(T[:3, 3]), self.origin if origin is None else origin,
                                                      self.margin if margin is None else margin, self.cursor)
        self.removed += removed
        self.cleared += removed
        return removed

    def frame(self, cloud, T, attr=None):
        """as P.RefDrive.frame, with the clearing between the fold and the range prune (a)"""
        radius = self.radius
        pos = np.array(np.asarray(T, np.float64)[:3, 3])
        if radius > 0.0 and not self.overflowed and self.made and self.last is not None and self.map.size + cloud.shape[0] > self.map.max_rows:
            self.prune(self.last)  # (b)
            self.center = self.last
        self.radius = 0.0  # the fold alone: policy (a) comes behind the clearing
        try:
            added = super().frame(cloud, T, attr)
        finally:
            self.radius = radius
        if added is not None:
            if self.clearing:
                self.clear_rays(cloud, T)
            if radius > 0.0:
                d = pos - (pos if self.center is None else self.center)
                step = radius / 4.0
                if self.center is None:
                    self.center = pos
                elif d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]) >= step * step:
                    self.prune(pos)
                    self.center = pos
        return added
