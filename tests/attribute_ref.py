"""The per-point attribute of include/madicp_hip.h (madicp_cloud_ingest_sources_attr, madicp_cloud_export_f32_attr,
madicp_map_create_attr ...) restated in numpy on top of the restatements the geometry already has.

TEST INFRASTRUCTURE ONLY.  The attribute is one uint32 word per point: the bytes of one record field, little-endian, zero-extended.
It is only ever copied, so every rule is "the word of the point the geometry's rule picks":

    words(records, off, code)        the word of EVERY record: its width bytes at `off`, zero-extended
    ingest(sources, t_range)         ingest_sources_ref.reference + the survivors' words, source 0's first
    export(xyz, attr, R, t, voxel)   cloud_export_ref.export_f32 + the words of the rows it keeps
    AttrMap                          voxel_map_ref.RefMap + the column: a row's word is its owning point's, 0 for a cloud without one
    with_attribute(sources, ...)     the sources of a case with an attribute field of one type at an UNALIGNED offset
"""
import copy

import numpy as np

import cloud_export_ref as E
import ingest_sources_ref as S
import voxel_map_ref as V
from mad_icp_amd.records import ATTR_DTYPE, RecordLayout

WIDTH = {code: dt.itemsize for code, dt in ATTR_DTYPE.items()}
CODES = sorted(ATTR_DTYPE)  # 1 .. 7


def words(records, off, code):
    """(n,) uint32: byte-wise, never through a typed view of the record (the field sits at any alignment)"""
    buf = np.ascontiguousarray(records)
    n = buf.shape[0]
    raw = buf.view(np.uint8).reshape(n, -1)
    w = np.zeros(n, np.uint32)
    for b in range(WIDTH[code]):
        w |= raw[:, off + b].astype(np.uint32) << np.uint32(8 * b)
    return w


def keep_mask(src):
    lay = RecordLayout(*src.layout)
    xyz, _ = S.R.fields(src.records, lay)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        nrm = np.sqrt(x * x + (y * y + z * z)).astype(np.float64)
        return ~((nrm < src.min_range) | (nrm > src.max_range) | np.isnan(x) | np.isnan(y) | np.isnan(z))


def ingest(sources, t_range=None):
    """(points, stamps or None, (t0, t1), survivors per source, words)"""
    pts, st, rng, per = S.reference(sources, t_range)
    w = np.concatenate([words(src.records, *src.attribute)[keep_mask(src)] for src in sources])
    assert w.shape[0] == pts.shape[0]
    return pts, st, rng, per, w


def unaligned_offset(lay, code, k=0):
    """an offset for a field of type `code` in layout `lay` that no load of the field's width could use: odd for the 2- and
    4-byte types (k varies it); always inside the record"""
    width = WIDTH[code]
    room = lay.point_step - width
    off = (1 + 2 * k) % (room + 1)
    if width > 1 and off % 2 == 0:
        off = max(1, off - 1) if room >= 1 else 0
    return min(off, room)


def with_attribute(sources, code, last_bytes=False):
    """copies of `sources` that name an attribute field of type `code`: at an unaligned offset, or in the record's last bytes"""
    out = []
    for k, src in enumerate(sources):
        lay = RecordLayout(*src.layout)
        s = copy.copy(src)
        s.attribute = (lay.point_step - WIDTH[code], code) if last_bytes else (unaligned_offset(lay, code, k), code)
        out.append(s)
    return out


def export(xyz, attr, R, t, voxel):
    q = E.positions(xyz, R, t)
    idx = E.kept_indices(q, voxel)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(q[idx].astype(np.float32)), np.ascontiguousarray(np.asarray(attr, np.uint32)[idx])


def hashed(n, seed=0):
    """a word per index that is no function of anything the geometry could reproduce by accident (Knuth's multiplicative hash)"""
    return ((np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)


class AttrMap(V.RefMap):
    """RefMap with the column: insert(cloud, attr or None, R, t)"""

    def __init__(self, voxel, max_rows=1 << 30):
        super().__init__(voxel, max_rows)
        self.words = []

    def insert(self, cloud, attr, R, t):
        before = set(self.keys)
        added = super().insert(cloud, R, t)
        if added is None:
            return None
        # the owners of the new rows, found again from the keys that were new: the lowest index of each, ascending
        q = E.positions(cloud, R, t)
        with np.errstate(all="ignore"):
            f = np.floor(q / self.voxel)
            cand = np.all((f >= -E.CELL) & (f < E.CELL), axis=1)
        idx = np.nonzero(cand)[0]
        owners, seen = [], set()
        if idx.size:
            k = f[idx].astype(np.int64) + int(E.CELL)
            key = k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)
            for i, kk in zip(idx.tolist(), key.tolist()):
                if kk not in before and kk not in seen:
                    seen.add(kk)
                    owners.append(i)
        assert len(owners) == added
        a = np.zeros(q.shape[0], np.uint32) if attr is None else np.asarray(attr, np.uint32)
        self.words.append(a[owners])
        return added

    def attr(self, first_row=0):
        w = np.concatenate(self.words) if self.words else np.empty(0, np.uint32)
        return np.ascontiguousarray(w[first_row:])

    def clear(self):
        super().clear()
        self.words = []
