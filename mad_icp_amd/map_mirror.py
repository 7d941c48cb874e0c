"""The reference consumer of a voxel map that reports its removals (Pipeline.setMapTrackRemoved): a host-side copy that stays
equal to the map from two small fetches per poll — the rows that have left, then the rows that are new.  numpy only.

A row's identity is its stored 64-bit voxel key (csrc/common/export_point.h: export_key): unique among the rows the map holds,
unchanged by a prune, which moves rows down, and not recoverable from the float row, which is rounded after the key is taken.
"""
import numpy as np

_CELL_BITS = 21
_CELL_MASK = (1 << _CELL_BITS) - 1
_CELL_OFFSET = 1 << 20


def key_cells(keys):
    """The voxel cells of stored keys: (n, 3) int32, each in [-2^20, 2^20) — the inverse of export_key's packing, 21 bits per
    axis, x lowest, every cell offset by 2^20."""
    k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    out = np.empty((k.shape[0], 3), np.int32)
    for i in range(3):
        out[:, i] = ((k >> np.uint64(_CELL_BITS * i)) & np.uint64(_CELL_MASK)).astype(np.int64) - _CELL_OFFSET
    return out


class MapMirror:
    """key -> (row, word) of a Pipeline's map.  update(pipe) applies one poll: pipe.mapRemovedRows() out, then
    pipe.mapNewRows(with_keys=True) in — in that order, a voxel that was cleared and refilled between two polls is in both lists.
    Afterwards keys() / rows() / attr(), sorted by key, are the map's (mapKeys(), mapCloud(), mapAttribute()) sorted by key, for
    any polling cadence.  The Pipeline must have setMapTrackRemoved(True) from before the first row is fetched."""

    def __init__(self, with_attribute=False):
        self.with_attribute = bool(with_attribute)
        self._rows = {}
        self._attr_dtype = np.dtype(np.uint32)

    def __len__(self):
        return len(self._rows)

    def update(self, pipe):
        """One poll.  Returns (rows removed, rows added).  KeyError for a removed key the mirror does not hold, ValueError for a
        new key it already holds: either means that rows were fetched some other way, or that tracking was off for a while."""
        gone = pipe.mapRemovedRows(with_attribute=self.with_attribute)
        new = pipe.mapNewRows(with_attribute=self.with_attribute, with_keys=True)
        removed = np.asarray(gone[0], dtype=np.uint64)
        for k in removed.tolist():
            if k not in self._rows:
                raise KeyError("MapMirror: removed key %d is not in the mirror" % k)
            del self._rows[k]
        xyz = np.asarray(new[0], dtype=np.float32).reshape(-1, 3)
        keys = np.asarray(new[-1], dtype=np.uint64)
        words = None
        if self.with_attribute:
            words = np.asarray(new[1])
            if words.shape[0]:
                self._attr_dtype = words.dtype
        for j, k in enumerate(keys.tolist()):
            if k in self._rows:
                raise ValueError("MapMirror: new key %d is already in the mirror" % k)
            self._rows[k] = (xyz[j].copy(), words[j] if words is not None else None)
        return removed.shape[0], keys.shape[0]

    def keys(self):
        return np.array(sorted(self._rows), dtype=np.uint64)

    def rows(self):
        out = np.empty((len(self._rows), 3), np.float32)
        for j, k in enumerate(sorted(self._rows)):
            out[j] = self._rows[k][0]
        return out

    def attr(self):
        if not self.with_attribute:
            raise RuntimeError("MapMirror: made without the attribute")
        out = np.empty(len(self._rows), self._attr_dtype)
        for j, k in enumerate(sorted(self._rows)):
            out[j] = self._rows[k][1]
        return out
