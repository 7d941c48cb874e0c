"""The voxel-map rule of include/madicp_hip.h (madicp_map_*) restated in numpy on top of cloud_export_ref.positions, with a Python
set of keys, and the sequences the host and the device tests share.  A map has a voxel size, M float32 rows and the set K of
their keys.  Folding a cloud through (R, t), everything in float64:
  position   q = cloud_export_ref.positions(cloud, R, t)
  candidate  cell = floor(q / voxel) per axis, -2^20 <= cell < 2^20 on all three (NaN / inf fail)
  key        (kx + 2^20) | (ky + 2^20) << 21 | (kz + 2^20) << 42 — from the float64 position, never from the stored float
  new        a candidate whose key is not in K; of the new points that share a key the LOWEST index is kept
  append     float32(q[i]) of the kept points in ascending index order; their keys join K"""
import numpy as np

import cloud_export_ref as E


class RefMap:
    def __init__(self, voxel, max_rows=1 << 30):
        self.voxel = float(voxel)
        self.max_rows = int(max_rows)
        self.keys = set()
        self.chunks = []
        self.size = 0

    def insert(self, cloud, R, t):
        """Returns the rows added; None (map unchanged) where the real thing refuses for capacity."""
        q = E.positions(cloud, R, t)
        n = q.shape[0]
        if self.size + n > self.max_rows:
            return None
        with np.errstate(all="ignore"):
            f = np.floor(q / self.voxel)
            cand = np.all((f >= -E.CELL) & (f < E.CELL), axis=1)
        idx = np.nonzero(cand)[0]
        kept = []
        if idx.size:
            k = f[idx].astype(np.int64) + int(E.CELL)
            key = k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)
            for i, kk in zip(idx.tolist(), key.tolist()):  # ascending index: the first arrival of a key is its lowest index
                if kk not in self.keys:
                    self.keys.add(kk)
                    kept.append(i)
        with np.errstate(all="ignore"):
            self.chunks.append(np.ascontiguousarray(q[kept].astype(np.float32)).reshape(-1, 3))
        self.size += len(kept)
        return len(kept)

    def rows(self, first_row=0):
        allrows = np.concatenate(self.chunks, axis=0) if self.chunks else np.empty((0, 3), np.float32)
        return np.ascontiguousarray(allrows[first_row:])

    def clear(self):
        self.keys.clear()
        self.chunks = []
        self.size = 0


SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
VOXEL = 0.5


def pose_of(kind, frame):
    """the pose of frame `frame` of a sequence: the identity, or a different rigid motion for every frame"""
    return E.IDENTITY if kind == "identity" else E.random_pose(40 + frame)


def sequence(n, seed):
    """3-6 frames of n points drawn from cloud_export_ref.input_sets: [(name, points)].  The draw wraps around the seven sets, so
    over the sizes every set is folded, some twice in one sequence (a repeated one_cell / own_cells / two_cells frame adds 0
    under the identity)."""
    frames = 3 + seed % 4
    sets = [E.input_sets(n, seed + 10 * f) for f in range(frames)]
    return [sets[f][(seed + 3 * f) % 7] for f in range(frames)]


_cache = {}


def reference(n, kind, voxel=VOXEL):
    """the restatement folded over sequence(n, 100 + n) under `kind` poses, computed once: [(points, R, t, added, rows after)]"""
    k = (n, kind, voxel)
    if k not in _cache:
        ref, out = RefMap(voxel), []
        for f, (_, pts) in enumerate(sequence(n, 100 + n)):
            R, t = pose_of(kind, f)
            added = ref.insert(pts, R, t)
            rows = ref.rows()
            rows.setflags(write=False)
            out.append((pts, R, t, added, rows))
        _cache[k] = out
    return _cache[k]
