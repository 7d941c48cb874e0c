"""The moments of the voxel map (include/madicp_hip.h: madicp_map_create_mom; the rule is csrc/common/voxel_moments.h's) restated in
numpy and Python integers on top of map_evidence_ref.RefEvidenceMap — which is map_removed_ref / map_clear_ref / map_prune_ref's
fold, prune, clearing, removal log and evidence word (a moments map without evidence runs it at 1/1/1, which is the plain map) —
and the sequences and the replay the host and the device tests share.
  offset    of a candidate position q: d = q / voxel, u = d - floor(d), w = min(floor(u * 65536), 65535) per axis
  moments   ten exact integers per row, n | S1[3] | S2[6] (xx, xy, xz, yy, yz, zz), over the candidate points the row has taken
  freeze    a row takes ALL candidate points of a fold that carry its stored key iff its n before that fold is < max_count
  removal   the ten words travel with their row; the removal log carries none
  surfel    centroid ((cell + (S1 / n + 0.5) / 65536) * voxel as float32) and the fp64 covariance S2 / n - m m^T from the integers
Steps are those of map_removed_ref."""
import numpy as np

import cloud_export_ref as E
import map_clear_ref as Cl
import map_evidence_ref as Ev
import map_removed_ref as Rm

VOXEL = Ev.VOXEL
MAX_COUNT_MAX = 2 ** 31
PAIRS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def refused(max_count):
    """what map_moments_refusal refuses"""
    return max_count < 1 or max_count > MAX_COUNT_MAX


def offsets(q, voxel):
    """the quantised in-voxel offsets (m, 3) int64 of CANDIDATE positions q (m, 3)"""
    d = q / np.float64(voxel)
    u = d - np.floor(d)
    return np.minimum(np.floor(u * 65536.0), 65535.0).astype(np.int64)


class RefMomentsMap(Ev.RefEvidenceMap):
    def __init__(self, voxel, max_count, params=None, max_rows=1 << 30, tracking=False):
        assert not refused(max_count)
        super().__init__(voxel, *(params or (1, 1, 1)), max_rows=max_rows, tracking=tracking)
        self.params, self.max_count = params, int(max_count)
        self.mom = []  # per row: ten Python integers

    def insert(self, cloud, R, t, attr=None):
        n_before = [m[0] for m in self.mom]
        added = super().insert(cloud, R, t, attr)
        if added is None:
            return None
        q = E.positions(cloud, R, t)
        cand, keys = Cl.keys_of(q, self.voxel)
        w = offsets(q[cand], self.voxel)
        self.mom += [[0] * 10 for _ in range(added)]
        n_before += [0] * added  # (the creating point is one of the points its row takes)
        row_of = {k: r for r, k in enumerate(self.row_keys.tolist())}
        for k, p in zip(keys.tolist(), w.tolist()):
            r = row_of[k]
            if n_before[r] >= self.max_count:
                continue
            m = self.mom[r]
            m[0] += 1
            for a in range(3):
                m[1 + a] += p[a]
            for j, (a, b) in enumerate(PAIRS):
                m[4 + j] += p[a] * p[b]
        return added

    def _remove(self, keep, watermark):
        mom = [m for m, k in zip(self.mom, keep.tolist()) if k]
        ans = super()._remove(keep, watermark)
        self.mom = mom
        return ans

    def moments(self, first_row=0):
        assert all(0 <= v < 2 ** 64 for m in self.mom for v in m)
        return np.array(self.mom[first_row:], dtype=np.uint64).reshape(-1, 10)

    def clear(self):
        self.__init__(self.voxel, self.max_count, self.params, self.max_rows, self.tracking)


def centroids(mom, keys, voxel):
    """the centroid rule in fp64, rounded to float32: (M, 3)"""
    out = np.empty((mom.shape[0], 3), np.float32)
    for r, (m, key) in enumerate(zip(mom.tolist(), keys.tolist())):
        for a in range(3):
            cell = np.float64(((int(key) >> (21 * a)) & 0x1fffff) - 2 ** 20)
            mean = np.float64(float(m[1 + a])) / np.float64(float(m[0]))
            out[r, a] = np.float32((cell + (mean + np.float64(0.5)) / np.float64(65536.0)) * np.float64(voxel))
    return out


def covariances(mom):
    """the fp64 covariance S2 / n - m m^T of every row, formed from the exact integers: (M, 3, 3), in offset units squared"""
    C = np.empty((mom.shape[0], 3, 3))
    for r, m in enumerate(mom.tolist()):
        n = float(m[0])
        mean = [float(m[1 + a]) / n for a in range(3)]
        for j, (a, b) in enumerate(PAIRS):
            C[r, a, b] = C[r, b, a] = float(m[4 + j]) / n - mean[a] * mean[b]
    return C


def eigh_surfels(mom, voxel):
    """numpy.linalg.eigh on covariances(): (eigenvalues in m^2 ascending (M, 3) fp64, normals (M, 3) fp64)"""
    w, V = np.linalg.eigh(covariances(mom))
    s = voxel / 65536.0
    return w * (s * s), V[:, :, 0]


def gap_ok(eig, count):
    """the rows a normal is compared on: n >= 3 and eigenvalue gap w1 - w0 >= 1e-3 w2; (mask, share of the n >= 3 rows left out)"""
    eig = np.asarray(eig, np.float64)
    full = count >= 3
    ok = full & (eig[:, 1] - eig[:, 0] >= 1e-3 * eig[:, 2])
    return ok, 1.0 - np.count_nonzero(ok) / max(np.count_nonzero(full), 1)


def sign_free_diff(a, b):
    """the worst component difference of unit vectors a, b (M, 3), modulo sign, per row"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1))


# ---- the sequences ----------------------------------------------------------------------------------------------------------------
CLOUD_SIZES = Ev.CLOUD_SIZES
ROW_NAMES = ["rows:%d" % m for m in (1023, 1024, 1025)]  # one below, at and one above the 1 024-mark scan tile


def one_voxel_top(n=4096):
    """n points in ONE voxel, all at w = 65535 on every axis, in one fold: n = 4096, S1 = 4096 x 65535, S2 = 4096 x 65535^2"""
    I, z = E.IDENTITY
    p = np.nextafter(np.array([10.5, 10.5, 5.5]), 0.0)  # (the last double below the voxel's far corner: u * 65536 > 65535)
    return [("fold", np.tile(p, (n, 1)), I, z)]


def crossing(n=4096):
    """the freeze crossing INSIDE a fold (max_count = 100): one voxel, a fold of n points takes all n, the next fold none; a second
    voxel with 60 + 60 + 60 points takes the first two folds (60 < 100, 120) and not the third"""
    I, z = E.IDENTITY
    rng = np.random.default_rng(5)
    a = np.array([10.25, 10.25, 5.25]) + rng.uniform(-0.2, 0.2, size=(n, 3))
    b = np.array([20.25, 0.25, 0.25]) + rng.uniform(-0.2, 0.2, size=(60, 3))
    return [("fold", np.concatenate([a, b]), I, z), ("fold", np.concatenate([b, a[:50]]), I, z), ("fold", b[::-1], I, z)]


def four_four_four():
    """folds of 4, 4, 4 points into one voxel: max_count = 5 gives n = 4, 8, 8"""
    I, z = E.IDENTITY
    rng = np.random.default_rng(9)
    pts = np.array([1.25, 1.25, 1.25]) + rng.uniform(-0.2, 0.2, size=(12, 3))
    return [("fold", pts[:4], I, z), ("fold", pts[4:8], I, z), ("fold", pts[8:], I, z)]


def wrapping():
    """map_evidence_ref.wrapping_cloud in a table of 128 slots: folds, a clearing, the cloud reversed, more clearings"""
    I, z = E.IDENTITY
    pts = Ev.wrapping_cloud(32, 128)
    rays = Cl.through(pts[::2], Cl.ORIGIN, np.full(16, 1.6))
    return [("fold", pts, I, z), ("fold", pts, I, z), ("clear", rays, I, z, Cl.ORIGIN, 0.0, 16), ("fold", pts[::-1], I, z),
            ("clear", rays, I, z, Cl.ORIGIN, 0.0, "all"), ("fold", pts[:9], I, z)]


def named(name):
    own = {"one_voxel_top": one_voxel_top, "crossing": crossing, "four_four_four": four_four_four, "wrapping": wrapping}
    return own[name]() if name in own else Ev.named(name)


def planes(points_per_plane=6000, noise=0.01, seed=0):
    """planted noisy planes of the fixtures.four_walls kind — four walls and a floor, 4 m wide, 2 m high, Gaussian noise across each
    plane — taken through a pose off every axis: (points (5 p, 3), R, t)"""
    rng = np.random.default_rng(100 + seed)
    w, h = 4.0, 2.0
    spans = [((0, w), (0, 0), (0, h)), ((0, w), (w, w), (0, h)), ((0, 0), (0, w), (0, h)), ((w, w), (0, w), (0, h)), ((0, w), (0, w), (0, 0))]
    out = []
    for span in spans:
        cols = [rng.uniform(lo, hi, points_per_plane) if hi > lo else lo + rng.normal(0.0, noise, points_per_plane) for lo, hi in span]
        out.append(np.column_stack(cols))
    R, t = E.random_pose(77 + seed)
    return np.vstack(out), R, t


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def run_ref(steps, max_count, params=None, voxel=VOXEL, max_rows=1 << 30, tracking=True, watermark="own"):
    """the restatement over `steps`: (steps with their watermarks resolved, [(answer, rows, keys, words, evidence, log count, taken,
    moments)]) — as map_evidence_ref.run_ref, with the ten words"""
    ref, done, out = RefMomentsMap(voxel, max_count, params, max_rows=max_rows, tracking=tracking), [], []
    for step in steps:
        ans = taken = None
        if step[0] == "fold":
            _, pts, R, t = step
            added = ref.insert(pts, R, t, np.arange(pts.shape[0], dtype=np.uint32))
            ans = None if added is None else (added, ref.size)
        elif step[0] == "prune":
            step = ("prune", step[1], step[2], Rm.resolve(step[3], ref.size, watermark))
            ans = ref.prune(*step[1:])
        elif step[0] == "clear":
            step = step[:6] + (Rm.resolve(step[6], ref.size, watermark),)
            ans = ref.clear_rays(*step[1:])
        elif step[0] == "take":
            taken = _frozen(*ref.take()) if ref.tracking else None
        elif step[0] == "track":
            ref.track(step[1])
        elif step[0] == "reset":
            ref.clear()
        else:
            raise ValueError(step[0])
        rows, keys, words, ev, mom = _frozen(ref.rows(), ref.stored_keys(), ref.attr(), ref.evidence(), ref.moments())
        assert mom.shape == (rows.shape[0], 10) and (mom.size == 0 or mom[:, 0].min() >= 1)
        done.append(step)
        out.append((ans, rows, keys, words, ev, ref.removed_count, taken, mom))
    return done, out


_cache = {}


def expected(name, max_count, params=None, tracking=True):
    """run_ref over named(name), computed once per combination"""
    k = (name, max_count, params, tracking)
    if k not in _cache:
        _cache[k] = run_ref(named(name), max_count, params, tracking=tracking)
    return _cache[k]


def replay(done, want, *impls, tag=""):
    """runs the resolved steps through every impl — map_evidence_ref.replay's interface and moments() (None on a map without them:
    not compared) — and holds each to the restatement after EVERY step: answer, rows, keys, words, evidence, the log's count, a
    take's content, and all ten moment words of every row, bit for bit"""
    for i, (step, (ans, rows, keys, words, ev, log_n, taken, mom)) in enumerate(zip(done, want)):
        for m in impls:
            at = (tag, i, step[0], type(m).__name__)
            if step[0] == "fold":
                got = m.insert(step[1], step[2], step[3], np.arange(step[1].shape[0], dtype=np.uint32))
                assert (None if got is None else tuple(got)) == ans, at + (got, ans)
            elif step[0] == "prune":
                got = m.prune(step[1], step[2], step[3])
                assert (None if got is None else tuple(got)) == ans, at + (got, ans)
            elif step[0] == "clear":
                got = m.clear_rays(*step[1:])
                assert (None if got is None else tuple(got)) == ans, at + (got, ans)
            elif step[0] == "take":
                if taken is not None:
                    assert Rm.same_log(m.take(), taken, m.words() is not None), at
            elif step[0] == "track":
                m.track(step[1])
            elif step[0] == "reset":
                m.reset()
            mine = m.rows()
            assert mine.dtype == np.float32 and mine.shape == rows.shape and E.same_bits(mine, rows), at
            k = m.keys()
            assert k.dtype == np.uint64 and k.tobytes() == keys.tobytes(), at
            w = m.words()
            if w is not None:
                assert w.dtype == np.uint32 and w.tobytes() == words.tobytes(), at
            e = m.evidence()
            if e is not None:
                assert e.dtype == np.uint32 and e.tobytes() == ev.tobytes(), at + (e, ev)
            g = m.moments()
            if g is not None:
                assert g.dtype == np.uint64 and g.shape == mom.shape, at + (g.shape, mom.shape)
                assert g.tobytes() == mom.tobytes(), at + (np.argwhere(g != mom)[:4].tolist(),)
            assert m.removed_count() == log_n, at + (m.removed_count(), log_n)
    return want


# ---- Pipeline's side of it --------------------------------------------------------------------------------------------------------
class RefDrive(Rm.RefDrive):
    """setMapAccumulation(moments=max_count[, evidence=]) + setMapClearing + setMapRange restated: map_removed_ref's drive over a
    RefMomentsMap — the frame order stays fold, clearing, range prune"""

    def __init__(self, voxel, max_count, params=None, radius=0.0, max_points=1 << 24, clearing=True, margin=0.0, origin=(0.0, 0.0, 0.0),
                 tracking=False):
        super().__init__(voxel, radius, max_points, clearing, margin, origin, tracking)
        self.map = RefMomentsMap(voxel, max_count, params, max_rows=max_points, tracking=tracking)
