"""The removal log of the voxel map (include/madicp_hip.h: madicp_map_track_removed / _take_removed) restated in numpy on top of
map_clear_ref.RefClearMap, which already keeps every row's stored key and word — and the replay the host and the device tests
share.  On a tracking map a prune or a clearing appends, in row order, the rows it removes from BELOW its watermark:
  log     += (row_keys[j], xyz[j], words[j]) for j < watermark with keep[j] false
  take()  returns the entries, oldest first, and empties the log
  full    a prune or a clearing while the log holds >= max_rows entries is refused (None), nothing changed
The step lists are those of map_prune_ref.named() and map_clear_ref.named(): ("fold", ...), ("prune", ...), ("clear", ...); the
replay adds ("take",) and ("track", on)."""
import numpy as np

import cloud_export_ref as E
import map_clear_ref as Cl
import map_prune_ref as P

VOXEL = P.VOXEL


class RefRemovedMap(Cl.RefClearMap):
    def __init__(self, voxel, max_rows=1 << 30, tracking=True):
        super().__init__(voxel, max_rows)
        self.tracking = bool(tracking)
        self._empty_log()

    def _empty_log(self):
        self.log_keys = np.empty(0, np.uint64)
        self.log_xyz = np.empty((0, 3), np.float32)
        self.log_words = np.empty(0, np.uint32)

    @property
    def removed_count(self):
        return self.log_keys.shape[0]

    def track(self, on):
        self.tracking = bool(on)
        if not on:
            self._empty_log()

    def _full(self):
        return self.tracking and self.removed_count >= self.max_rows

    def _remove(self, keep, watermark):
        assert 0 <= watermark <= self.size
        before = self.size
        mark = int(np.count_nonzero(keep[:watermark]))
        if self.tracking:
            gone = ~keep
            gone[watermark:] = False  # rows at or above the watermark were never delivered
            self.log_keys = np.concatenate([self.log_keys, self.row_keys[gone].astype(np.uint64)])
            self.log_xyz = np.concatenate([self.log_xyz, self.xyz[gone]], axis=0)
            self.log_words = np.concatenate([self.log_words, self.words[gone]])
        for kk in self.row_keys[~keep].tolist():
            self.keys.remove(kk)
        self.xyz, self.row_keys, self.words = self.xyz[keep], self.row_keys[keep], self.words[keep]
        return before - self.size, self.size, mark

    def prune(self, center, radius, watermark=0):
        """(removed, rows, watermark); None (nothing changed) where the real thing refuses because the log is full"""
        if self._full():
            return None
        return self._remove(self.kept_mask(center, radius), watermark)

    def clear_rays(self, cloud, R, t, origin=(0.0, 0.0, 0.0), margin=0.0, watermark=0):
        if self._full():
            return None
        keep = ~self.cleared_mask(cloud, R, t, origin, margin) if self.size else np.zeros(0, bool)
        return self._remove(keep, watermark)

    def take(self):
        out = (self.log_keys, self.log_xyz, self.log_words)
        self._empty_log()
        return out

    def stored_keys(self):
        return self.row_keys.astype(np.uint64)

    def clear(self):
        tracking = self.tracking
        self.__init__(self.voxel, self.max_rows, tracking)


def steps_of(name):
    """the step list of a name of either module: "prune:<name>" or "clear:<name>" """
    kind, _, rest = name.partition(":")
    return {"prune": P.named, "clear": Cl.named}[kind](rest)


WATERMARKS = ["own", "0", "1", "half", "last", "all"]


def resolve(wm, size, mode="own"):
    """the watermark of a step: the step's own (an int, a fraction of the rows, "all"), or what `mode` puts in its place"""
    if mode == "own":
        return size if wm == "all" else (int(wm * size) if isinstance(wm, float) else min(wm, size))
    return {"0": 0, "1": min(1, size), "half": size // 2, "last": max(size - 1, 0), "all": size}[mode]


def with_takes(steps, cadence):
    """("take",) behind every step ("every"), or one behind the last ("end"); "never": none"""
    if cadence == "never":
        return list(steps)
    if cadence == "end":
        return list(steps) + [("take",)]
    out = []
    for s in steps:
        out += [s, ("take",)]
    return out


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def run_ref(steps, voxel=VOXEL, max_rows=1 << 30, tracking=True, watermark="own"):
    """the restatement over `steps`: (steps with their watermarks resolved, [(answer, rows, keys, words, log count, taken)]) —
    answer: the step's own, None for a refused removal and for "take" / "track"; taken: (keys, rows, words) of a "take", else None.
    A fold's points carry their index as attribute word."""
    ref, done, out = RefRemovedMap(voxel, max_rows, tracking), [], []
    for step in steps:
        ans = taken = None
        if step[0] == "fold":
            _, pts, R, t = step
            added = ref.insert(pts, R, t, np.arange(pts.shape[0], dtype=np.uint32))
            ans = None if added is None else (added, ref.size)
        elif step[0] == "prune":
            _, c, r, wm = step
            step = ("prune", c, r, resolve(wm, ref.size, watermark))
            ans = ref.prune(*step[1:])
        elif step[0] == "clear":
            _, pts, R, t, o, margin, wm = step
            step = ("clear", pts, R, t, o, margin, resolve(wm, ref.size, watermark))
            ans = ref.clear_rays(*step[1:])
        elif step[0] == "take":
            taken = _frozen(*ref.take()) if ref.tracking else None
        elif step[0] == "track":
            ref.track(step[1])
        elif step[0] == "reset":
            ref.clear()
        else:
            raise ValueError(step[0])
        rows, keys, words = _frozen(ref.rows(), ref.stored_keys(), ref.attr())
        done.append(step)
        out.append((ans, rows, keys, words, ref.removed_count, taken))
    return done, out


_cache = {}


def expected(name, cadence="every", watermark="own", tracking=True):
    """run_ref over steps_of(name) with the takes of `cadence`, computed once per combination"""
    k = (name, cadence, watermark, tracking)
    if k not in _cache:
        _cache[k] = run_ref(with_takes(steps_of(name), cadence), tracking=tracking, watermark=watermark)
    return _cache[k]


def same_log(got, want, with_attr):
    """a taken log (keys, rows[, words]) against the restatement's, bit for bit"""
    keys, rows = got[0], got[1]
    ok = keys.dtype == np.uint64 and keys.tobytes() == want[0].tobytes()
    ok = ok and rows.dtype == np.float32 and rows.shape == want[1].shape and E.same_bits(rows, want[1])
    if with_attr:
        ok = ok and got[2].dtype == np.uint32 and got[2].tobytes() == want[2].tobytes()
    return bool(ok)


def replay(done, want, *impls, tag=""):
    """runs the resolved steps through every impl — insert(points, R, t, words), prune(center, radius, watermark),
    clear_rays(points, R, t, origin, margin, watermark) (each: the answer tuple, None where refused for capacity), rows(), keys(),
    words() (None: no column), removed_count(), take() ((keys, rows[, words])), track(on), reset() — and holds each to the
    restatement after EVERY step: answer, rows, keys, words, the log's count, and a take's content."""
    for i, (step, (ans, rows, keys, words, log_n, taken)) in enumerate(zip(done, want)):
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
                    assert same_log(m.take(), taken, m.words() is not None), at
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
            assert m.removed_count() == log_n, at + (m.removed_count(), log_n)
    return want


class RefDrive(Cl.RefDrive):
    """Pipeline's side of it (setMapAccumulation + setMapClearing + setMapRange + setMapTrackRemoved) restated: map_clear_ref's
    drive over a RefRemovedMap — every removal passes the consumer's cursor as watermark, so the log is "delivered, now gone"."""

    def __init__(self, voxel, radius=0.0, max_points=1 << 24, clearing=True, margin=0.0, origin=(0.0, 0.0, 0.0), tracking=True):
        super().__init__(voxel, radius, max_points, clearing, margin, origin)
        self.map = RefRemovedMap(voxel, max_points, tracking)

    def new_rows_keyed(self):
        """what mapNewRows(with_attribute=True, with_keys=True) returns: (rows, words, keys)"""
        first = self.cursor
        rows, words = self.new_rows()
        return rows, words, self.map.stored_keys()[first:]

    def removed_rows(self):
        return self.map.take()
