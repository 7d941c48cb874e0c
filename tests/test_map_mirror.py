"""mad_icp_amd.map_mirror: key_cells against export_key's packing (csrc/common/export_point.h: 21 bits per axis, offset 2^20) at the
ends of the cell range, through the host voxel map's stored keys; MapMirror driven by a fake object with the three methods it
calls — removals before additions, KeyError on an unknown removed key, ValueError on a duplicate new key.  No GPU."""
import numpy as np
import pytest

import cloud_export_ref as E
from mad_icp_amd import capi
from mad_icp_amd.map_mirror import MapMirror, key_cells

LO, HI = -(1 << 20), (1 << 20) - 1


def packed(cells):
    c = np.asarray(cells, np.int64) + (1 << 20)
    return (c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)).astype(np.uint64)


def test_key_cells_inverts_the_packing_at_the_range_ends():
    cells = np.array([[LO, LO, LO], [HI, HI, HI], [LO, HI, 0], [HI, 0, LO], [0, LO, HI], [0, 0, 0], [-1, 1, -1], [123456, -654321, 7]])
    got = key_cells(packed(cells))
    assert got.dtype == np.int32 and got.shape == (8, 3) and np.array_equal(got, cells)
    assert key_cells(np.empty(0, np.uint64)).shape == (0, 3)
    assert packed([[HI, HI, HI]])[0] == (1 << 63) - 1  # bit 63 of a real key is never set


def test_key_cells_of_the_keys_a_map_stores(natives):
    """the keys the host map stores for points at the range ends (voxel 0.5: cell c holds 0.5 c + 0.25) are those cells"""
    voxel = 0.5
    cells = np.array([[LO, LO, LO], [HI, HI, HI], [LO, HI, 0], [HI, 0, LO], [3, -4, 5]])
    pts = cells * voxel + 0.25
    h = capi.host_map_create(voxel, 8, 64)
    try:
        assert capi.host_map_insert(h, np.concatenate([pts, [[(HI + 1) * voxel + 0.25, 0.0, 0.0]]]), *E.IDENTITY) == (5, 5)  # (one beyond)
        keys = capi.host_map_download_keys(h)
        assert keys.tobytes() == packed(cells).tobytes() and np.array_equal(key_cells(keys), cells)
        assert np.array_equal(np.floor(capi.host_map_download_f32(h).astype(np.float64) / voxel).astype(np.int64), cells)
    finally:
        capi.host_map_destroy(h)


class Fake:
    """what MapMirror.update asks of a Pipeline, from a script of polls: (removed keys, removed rows, new rows, new words, new keys)"""

    def __init__(self, polls):
        self.polls, self.calls = list(polls), []

    def mapRemovedRows(self, with_attribute=False):
        self.calls.append("removed")
        k, x = self.polls[0][0], self.polls[0][1]
        w = np.zeros(len(k), np.uint32)
        return (np.array(k, np.uint64), np.array(x, np.float32).reshape(-1, 3)) + ((w,) if with_attribute else ())

    def mapNewRows(self, with_attribute=False, with_keys=False):
        self.calls.append("new")
        _, _, x, w, k = self.polls.pop(0)
        assert with_keys
        return (np.array(x, np.float32).reshape(-1, 3),) + ((np.array(w, np.uint16),) if with_attribute else ()) + (np.array(k, np.uint64),)


def test_the_mirror_applies_removals_then_additions():
    fake = Fake([([], [], [[1, 1, 1], [2, 2, 2], [3, 3, 3]], [10, 20, 30], [7, 5, 9]),
                 # key 5 leaves and is filled again between two polls: it is in both lists, with another row and word
                 ([5, 9], [[2, 2, 2], [3, 3, 3]], [[4, 4, 4], [6, 6, 6]], [40, 60], [5, 2]),
                 ([], [], [], [], [])])
    m = MapMirror(with_attribute=True)
    assert m.update(fake) == (0, 3) and m.keys().tolist() == [5, 7, 9] and m.rows()[:, 0].tolist() == [2.0, 1.0, 3.0]
    assert m.attr().tolist() == [20, 10, 30] and m.attr().dtype == np.uint16  # (the field's dtype, as mapNewRows views it)
    assert m.update(fake) == (2, 2) and m.keys().tolist() == [2, 5, 7] and m.keys().dtype == np.uint64
    assert m.rows().tolist() == [[6.0] * 3, [4.0] * 3, [1.0] * 3] and m.rows().dtype == np.float32 and m.attr().tolist() == [60, 40, 10]
    assert m.update(fake) == (0, 0) and len(m) == 3
    assert fake.calls == ["removed", "new"] * 3  # removals are fetched, and applied, first
    plain = MapMirror()
    assert plain.update(Fake([([], [], [[1, 2, 3]], None, [1 << 62])])) == (0, 1) and plain.keys().tolist() == [1 << 62]
    with pytest.raises(RuntimeError):
        plain.attr()


def test_the_mirror_raises_on_an_unknown_removed_key():
    m = MapMirror()
    m.update(Fake([([], [], [[1, 1, 1]], None, [7])]))
    with pytest.raises(KeyError):
        m.update(Fake([([8], [[1, 1, 1]], [], None, [])]))
    with pytest.raises(KeyError):  # the same key twice in one poll: the second is unknown by then
        m.update(Fake([([7, 7], [[1, 1, 1], [1, 1, 1]], [], None, [])]))


def test_the_mirror_raises_on_a_duplicate_new_key():
    m = MapMirror()
    m.update(Fake([([], [], [[1, 1, 1]], None, [7])]))
    with pytest.raises(ValueError):
        m.update(Fake([([], [], [[2, 2, 2]], None, [7])]))
    with pytest.raises(ValueError):
        m.update(Fake([([], [], [[2, 2, 2], [3, 3, 3]], None, [8, 8])]))
    m2 = MapMirror()
    m2.update(Fake([([], [], [[1, 1, 1]], None, [7])]))
    assert m2.update(Fake([([7], [[1, 1, 1]], [[2, 2, 2]], None, [7])])) == (1, 1)  # removed first: not a duplicate
