"""The evidence column of the voxel map (include/madicp_hip.h: madicp_map_create_ev; the rule is csrc/common/export_point.h's)
restated in numpy on top of map_removed_ref.RefRemovedMap — which is map_clear_ref / map_prune_ref / voxel_map_ref's fold, prune,
clearing and removal log — and the sequences and the replay the host and the device tests share.  Integers only:
  fold      N = the candidate keys of the cloud; a row the fold creates gets e = hit; a row that was there before the fold and whose
            stored key is in N gets e = min(e + hit, cap), once per fold; other rows are not touched
  clearing  a row whose stored key is in T \\ O is missed: e > miss -> it stays with e - miss, else it leaves (the close-up, the
            watermark and the removal log of the plain map); rows in O and rows not in T are not touched
  prune     the word travels with its row;  confirmed(min_e): the rows with e >= min_e, in row order
Steps are those of map_removed_ref: ("fold", points, R, t), ("prune", center, radius, watermark), ("clear", points, R, t, origin,
margin, watermark), ("take",), ("track", on), ("reset",)."""
import numpy as np

import cloud_export_ref as E
import map_clear_ref as Cl
import map_prune_ref as P
import map_removed_ref as Rm

VOXEL = P.VOXEL
CAP_MAX = 2 ** 31 - 1


def refused(hit, miss, cap):
    """what map_evidence_refusal refuses"""
    return hit < 1 or miss < 1 or cap < hit or cap > CAP_MAX


class RefEvidenceMap(Rm.RefRemovedMap):
    def __init__(self, voxel, hit, miss, cap, max_rows=1 << 30, tracking=False):
        assert not refused(hit, miss, cap)
        super().__init__(voxel, max_rows, tracking)
        self.hit, self.miss, self.cap = int(hit), int(miss), int(cap)
        self.ev = np.empty(0, np.int64)

    def insert(self, cloud, R, t, attr=None):
        before = self.size
        _, n_keys = Cl.keys_of(E.positions(cloud, R, t), self.voxel)
        met = np.isin(self.row_keys, n_keys)  # the rows that are there BEFORE the fold
        added = super().insert(cloud, R, t, attr)
        if added is None:
            return None
        assert met.shape[0] == before and self.size == before + added
        self.ev[met] = np.minimum(self.ev[met] + self.hit, self.cap)
        self.ev = np.concatenate([self.ev, np.full(added, self.hit, np.int64)])
        return added

    def _remove(self, keep, watermark):
        ev = self.ev[keep]
        ans = super()._remove(keep, watermark)
        self.ev = ev
        return ans

    def clear_rays(self, cloud, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, watermark=0):
        if self._full():
            return None
        if not self.size:
            return self._remove(np.zeros(0, bool), watermark)
        missed = self.cleared_mask(cloud, R, t, origin, margin)
        stays = missed & (self.ev > self.miss)
        self.ev[stays] -= self.miss
        return self._remove(~missed | stays, watermark)

    def evidence(self, first_row=0):
        return np.ascontiguousarray(self.ev[first_row:].astype(np.uint32))

    def confirmed(self, min_e):
        """(rows, keys, words, evidence) of the rows with e >= min_e"""
        m = self.ev >= int(min_e)
        return (np.ascontiguousarray(self.xyz[m]), self.stored_keys()[m], np.ascontiguousarray(self.words[m]),
                self.ev[m].astype(np.uint32))

    def clear(self):
        self.__init__(self.voxel, self.hit, self.miss, self.cap, self.max_rows, self.tracking)


# ---- the sequences ----------------------------------------------------------------------------------------------------------------
CLOUD_SIZES = [1, 63, 64, 65, 257, 3000]
PARAMS = [(1, 1, 1), (1, 1, 8), (4, 1, 16), (3, 2, 7), (2, 5, 6)]


def mixed(n, seed=0):
    """folds, clearings and prunes over clouds of n points: a cloud twice (every row hit once), a shifted cloud (old and new voxels in
    one fold), a clearing that looks through some rows, beyond and into and short of them, the first cloud DIRECTLY behind it, the
    clearing again (what stayed with less is missed again), a prune, the shifted cloud DIRECTLY behind it, a clearing at a margin"""
    rng = np.random.default_rng(7000 + n + seed)
    R, t = E.random_pose(300 + n + seed)
    I, z = E.IDENTITY
    a = E.gaussian(n, 11 + n + seed, scale=6.0)
    b = np.concatenate([a[: (n + 1) // 2], a[n // 2:] + np.array([40.0, 0.0, 0.0])])
    rows = E.positions(a, R, t)
    pick = rows[rng.integers(0, n, size=max(n // 2, 1))]
    rays = Cl.through(pick, Cl.ORIGIN, rng.choice([1.6, 1.0, 0.5], size=pick.shape[0]))
    return [("fold", a, R, t), ("fold", a, R, t), ("fold", b, R, t), ("clear", rays, I, z, Cl.ORIGIN, 0.0, 0.5), ("fold", a, R, t),
            ("clear", rays, I, z, Cl.ORIGIN, 0.0, "all"), ("prune", np.array(t), 6.0, 0.5), ("fold", b, R, t),
            ("clear", rays, I, z, Cl.ORIGIN, 0.25, 0), ("take",)]


def rows_of(m, hits=2):
    """a map of exactly m rows (own_cells: one voxel each), folded `hits` times, looked through at every third row (twice, so that
    small words run out), folded again, and a clearing that removes nothing: the scan over m + 1 marks, the compaction"""
    I, z = E.IDENTITY
    cells = E.own_cells(m)
    rays = Cl.through(cells[::3], Cl.ORIGIN, np.full(cells[::3].shape[0], 1.6))
    return ([("fold", cells, I, z)] * hits +
            [("clear", rays, I, z, Cl.ORIGIN, 0.0, 0.5), ("clear", rays, I, z, Cl.ORIGIN, 0.0, "all"), ("fold", cells, I, z),
             ("clear", cells, I, z, Cl.ORIGIN, 0.0, 0)])


def one_voxel(n=4096):
    """n points in ONE voxel, three times: the row gets hit once, then + hit per fold — the election's contention worst case; with a
    second voxel that only the first fold sees"""
    I, z = E.IDENTITY
    rng = np.random.default_rng(3)
    pts = np.array([10.25, 10.25, 5.25]) + rng.uniform(-0.2, 0.2, size=(n, 3))
    first = np.concatenate([pts, [[50.25, 0.25, 0.25]]])
    return [("fold", first, I, z), ("fold", pts, I, z), ("fold", pts, I, z)]


def old_and_new():
    """a fold with both old and new voxels: the new rows get hit, the old ones + hit, the ones it does not touch nothing"""
    I, z = E.IDENTITY
    cells = E.own_cells(30)
    return [("fold", cells[:20], I, z), ("fold", np.concatenate([cells[10:], cells[10:15]]), I, z)]


def line(cells):
    return np.array([[0.5 * c + 0.25, 0.25, 0.25] for c in cells])


def see_through(times, hits=1):
    """voxels 1 .. 6 on a line along +x from the origin's voxel 0, folded `hits` times; then `times` clearings by ONE ray that ends
    in voxel 4: voxels 1 .. 3 are missed every time, voxel 4 is traversed (its last sample) AND occupied, 5 and 6 are not reached"""
    I, z = E.IDENTITY
    ray = np.array([[2.3, 0.25, 0.25]])
    return [("fold", line(range(1, 7)), I, z)] * hits + [("clear", ray, I, z, np.array([0.25, 0.25, 0.25]), 0.0, 3)] * times


def prune_in_front(n=300):
    """rows near the origin in FRONT of far rows with more evidence: the prune removes the near ones, the words follow their rows"""
    I, z = E.IDENTITY
    near, far = E.own_cells(n), E.own_cells(n) + np.array([500.0, 0.0, 0.0])
    return [("fold", near, I, z), ("fold", far, I, z), ("fold", far[::2], I, z), ("fold", far[::4], I, z),
            ("prune", np.array([500.0, 0.0, 0.0]), 200.0, n // 2), ("fold", far[1::2], I, z), ("fold", near[:7], I, z)]


def growths(frames=5, n=700):
    """frames that make a map of initial_rows = 1 grow at nearly every fold, every cloud overlapping the one before, with a clearing
    and a prune in between"""
    out = []
    I, z = E.IDENTITY
    for f in range(frames):
        R, t = E.random_pose(900 + f // 2)  # (two frames per pose: the second hits the first's rows)
        pts = E.gaussian(n, 400 + f // 2, scale=5.0 + f)
        out.append(("fold", pts, R, t))
        if f == 2:
            q = E.positions(pts, R, t)
            out.append(("clear", Cl.through(q[::5], Cl.ORIGIN, np.full(q[::5].shape[0], 1.5)), I, z, Cl.ORIGIN, 0.0, 0.5))
        if f == 3:
            out.append(("prune", np.array(t), 8.0, "all"))
    return out


def named(name):
    kind, _, rest = name.partition(":")
    if kind == "mixed":
        return mixed(int(rest))
    if kind == "rows":
        return rows_of(int(rest))
    if kind in ("prune", "clear"):
        return Rm.steps_of(name)
    return {"one_voxel": one_voxel, "old_and_new": old_and_new, "prune_in_front": prune_in_front, "growths": growths}[name]()


MIXED_NAMES = ["mixed:%d" % n for n in CLOUD_SIZES]
ROW_NAMES = ["rows:%d" % m for m in (1023, 1024, 1025, 2500)]  # one below, at and one above the 1 024-mark scan tile; across two
PLAIN_NAMES = ["prune:size-257-alternate", "prune:posed", "clear:size-1025-257", "clear:edges", "clear:protected", "clear:scene"]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def run_ref(steps, params, voxel=VOXEL, max_rows=1 << 30, tracking=True, watermark="own"):
    """the restatement over `steps`: (steps with their watermarks resolved, [(answer, rows, keys, words, evidence, log count,
    taken)]) — as map_removed_ref.run_ref, with the column"""
    ref, done, out = RefEvidenceMap(voxel, *params, max_rows=max_rows, tracking=tracking), [], []
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
        rows, keys, words, ev = _frozen(ref.rows(), ref.stored_keys(), ref.attr(), ref.evidence())
        assert ev.shape[0] == rows.shape[0] and (ev.size == 0 or (1 <= ev.min() and ev.max() <= ref.cap))
        done.append(step)
        out.append((ans, rows, keys, words, ev, ref.removed_count, taken))
    return done, out


_cache = {}


def expected(name, params, tracking=True):
    """run_ref over named(name), computed once per combination"""
    k = (name, tuple(params), tracking)
    if k not in _cache:
        _cache[k] = run_ref(named(name), params, tracking=tracking)
    return _cache[k]


def same_confirmed(got, rows, keys, words, ev, min_e, with_attr):
    """what download_min_evidence(min_e, keys, words?, evidence) returned against numpy filtering of the columns"""
    m = ev >= min_e
    ok = got[0].dtype == np.float32 and got[0].shape == rows[m].shape and E.same_bits(got[0], np.ascontiguousarray(rows[m]))
    ok = ok and got[1].dtype == np.uint64 and got[1].tobytes() == keys[m].tobytes()
    if with_attr:
        ok = ok and got[2].dtype == np.uint32 and got[2].tobytes() == words[m].tobytes()
    return bool(ok and got[-1].dtype == np.uint32 and got[-1].tobytes() == ev[m].tobytes())


def replay(done, want, *impls, tag="", cap=None):
    """runs the resolved steps through every impl — map_removed_ref.replay's interface and evidence() (None on a plain map: the
    column is then not compared) and confirmed(min_e) -> (rows, keys[, words], evidence) — and holds each to the restatement after
    EVERY step: answer, rows, keys, words, evidence, the log's count, a take's content; and, where `cap` is given, the filtered
    download at min_e = 0, 1, 2, cap and cap + 1 after the last step and the one in the middle."""
    for i, (step, (ans, rows, keys, words, ev, log_n, taken)) in enumerate(zip(done, want)):
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
                if cap is not None and i in (len(done) // 2, len(done) - 1):
                    for min_e in (0, 1, 2, cap, cap + 1):
                        assert same_confirmed(m.confirmed(min_e), rows, keys, words, ev, min_e, w is not None), at + (min_e,)
            assert m.removed_count() == log_n, at + (m.removed_count(), log_n)
    return want


# ---- a table small enough that probes wrap past its last slot ------------------------------------------------------------------------
def slot0(key, slots):
    """frontend.hip.h's export_slot0: where the probe of a key starts in a table of `slots` slots"""
    mask = (1 << 64) - 1
    h = int(key)
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & mask
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & mask
    h ^= h >> 33
    return ((h >> 32) * slots) >> 32


def wraps(keys, slots):
    """whether linear probing of these keys into `slots` slots runs past the last slot — whatever the order they arrive in: more keys
    start in [s, slots) than it has slots, for some s"""
    starts = np.bincount([slot0(k, slots) for k in keys], minlength=slots)
    tail = np.cumsum(starts[::-1])  # keys that start in the last 1, 2, ... slots
    return bool(np.any(tail > np.arange(1, slots + 1)))


def wrapping_cloud(n=32, slots=128):
    """n points in voxels of their own whose keys make a table of `slots` slots wrap (found by shifting a lattice along x)"""
    for shift in range(4096):
        pts = E.own_cells(n) + np.array([0.5 * shift, 0.0, 0.0])
        _, keys = Cl.keys_of(pts, VOXEL)
        if len(set(keys.tolist())) == n and wraps(keys.tolist(), slots):
            return pts
    raise AssertionError("no wrapping cloud found")


# ---- Pipeline's side of it --------------------------------------------------------------------------------------------------------
class RefDrive(Rm.RefDrive):
    """setMapAccumulation(evidence=(hit, miss, cap)) + setMapClearing + setMapRange restated: map_removed_ref's drive over a
    RefEvidenceMap — the frame order stays fold, clearing, range prune"""

    def __init__(self, voxel, params, radius=0.0, max_points=1 << 24, clearing=True, margin=0.0, origin=(0.0, 0.0, 0.0), tracking=False):
        super().__init__(voxel, radius, max_points, clearing, margin, origin, tracking)
        self.map = RefEvidenceMap(voxel, *params, max_rows=max_points, tracking=tracking)
