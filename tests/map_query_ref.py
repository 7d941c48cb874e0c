"""The map query (include/madicp_hip.h: madicp_map_query_cloud) restated in numpy, written without the hash table, and the
scenarios the host and the device tests share.  Everything in float64 or integers, elementwise (numpy does not fuse):
  q          point i through (R, t): cloud_export_ref.positions
  cell       floor(q / voxel) per axis; candidate iff -2^20 <= cell < 2^20 on all three (NaN / inf fail)
  N(i)       the rows whose STORED key's cells — the key taken apart, 21 bits per axis — differ from the point's by at most `reach`
             per axis (a cell outside the key range has no key: nothing wraps)
  d2         dx dx + (dy dy + dz dz) with dx = q[0] - float64(row[0]) ...: from the stored float32 row
  answer     the row of N(i) with the smallest (d2, row); none: row -1, d2 +inf, key all ones, words 0
  counts     (candidates, rows >= 0, of those d2 <= max_dist * max_dist)
`query` finds N(i) by a sorted search of the 27 neighbour keys among the rows' keys; `query_brute` compares every point with every
row — the definition read literally, for small cases — and tests/test_host_map_query.py holds the first to the second."""
import itertools

import numpy as np

import cloud_export_ref as E

VOXEL = 0.5
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
HALF = 1 << 20
NONE = 1 << 31  # "no row yet": larger than every row


def cells_of(q, voxel):
    """(candidate mask, int64 cells (n, 3) — zeros where the point is no candidate)"""
    with np.errstate(all="ignore"):
        f = np.floor(q / voxel)
        cand = np.all((f >= -E.CELL) & (f < E.CELL), axis=1)
    cells = np.zeros(q.shape, np.int64)
    cells[cand] = f[cand].astype(np.int64)
    return cand, cells


def key_cells(keys):
    """the three cells of stored keys (m,) -> int64 (m, 3)"""
    k = np.asarray(keys, np.uint64).astype(np.int64)  # (bit 63 of a real key is never set)
    return np.stack([(k >> (21 * a)) & (2 * HALF - 1) for a in range(3)], axis=1) - HALF


def _d2(q, rows64):
    d = q - rows64
    return d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def _answer(q, cand, row, d2, keys, max_dist, attr, ev):
    matched = row != NONE
    row = np.where(matched, row, -1).astype(np.int32)
    j = np.where(matched, row, 0)
    m = keys.shape[0]
    out = {"row": row, "d2": d2,
           "keys": np.where(matched, keys[j] if m else NO_KEY, NO_KEY).astype(np.uint64) if q.shape[0] else np.zeros(0, np.uint64)}
    for name, col in (("attr", attr), ("ev", ev)):
        if col is not None:
            col = np.asarray(col, np.uint32)
            out[name] = np.where(matched, col[j] if m else 0, 0).astype(np.uint32)
    md2 = np.float64(max_dist) * np.float64(max_dist)
    out["counts"] = (int(np.count_nonzero(cand)), int(np.count_nonzero(matched)), int(np.count_nonzero(matched & (d2 <= md2))))
    return out


def query(rows, keys, cloud, R, t, voxel=VOXEL, reach=1, max_dist=np.inf, attr=None, ev=None):
    """rows (m, 3) float32 and keys (m,) uint64 as the map stores them; returns {"counts", "row", "d2", "keys"[, "attr"][, "ev"]}"""
    rows64 = np.asarray(rows, np.float32).reshape(-1, 3).astype(np.float64)
    keys = np.asarray(keys, np.uint64).reshape(-1)
    q = E.positions(cloud, R, t)
    n = q.shape[0]
    cand, cells = cells_of(q, voxel)
    best_row, best_d2 = np.full(n, NONE, np.int64), np.full(n, np.inf)
    order = np.argsort(keys.astype(np.int64), kind="stable")
    sorted_keys = keys.astype(np.int64)[order]
    for o in itertools.product(range(-reach, reach + 1), repeat=3):
        if keys.size == 0:
            break
        nb = cells + np.array(o, np.int64)
        idx = np.nonzero(cand & np.all((nb >= -HALF) & (nb < HALF), axis=1))[0]
        k = (nb[idx, 0] + HALF) | ((nb[idx, 1] + HALF) << 21) | ((nb[idx, 2] + HALF) << 42)
        at = np.minimum(np.searchsorted(sorted_keys, k), keys.size - 1)
        hit = sorted_keys[at] == k
        idx, j = idx[hit], order[at[hit]]
        with np.errstate(all="ignore"):
            d2 = _d2(q[idx], rows64[j])
            first = (d2 < best_d2[idx]) | ((d2 == best_d2[idx]) & (j < best_row[idx]))
        best_d2[idx[first]], best_row[idx[first]] = d2[first], j[first]
    return _answer(q, cand, best_row, best_d2, keys, max_dist, attr, ev)


def query_brute(rows, keys, cloud, R, t, voxel=VOXEL, reach=1, max_dist=np.inf, attr=None, ev=None):
    """the definition, one point at a time against every row"""
    rows64 = np.asarray(rows, np.float32).reshape(-1, 3).astype(np.float64)
    keys = np.asarray(keys, np.uint64).reshape(-1)
    row_cells = key_cells(keys)
    q = E.positions(cloud, R, t)
    n = q.shape[0]
    cand, cells = cells_of(q, voxel)
    best_row, best_d2 = np.full(n, NONE, np.int64), np.full(n, np.inf)
    for i in np.nonzero(cand)[0]:
        near = np.nonzero(np.all(np.abs(row_cells - cells[i]) <= reach, axis=1))[0]
        with np.errstate(all="ignore"):
            d2 = _d2(q[i][None], rows64[near])
        near, d2 = near[~np.isnan(d2)], d2[~np.isnan(d2)]
        if near.size:
            k = np.lexsort((near, d2))[0]
            best_row[i], best_d2[i] = near[k], d2[k]
    return _answer(q, cand, best_row, best_d2, keys, max_dist, attr, ev)


COLUMNS = ("row", "d2", "keys", "attr", "ev")


def same(got, want, tag=""):
    """got: (counts, row, d2[, keys][, attr][, ev]) as capi returns it, in COLUMNS' order of the columns `want` has"""
    names = [c for c in COLUMNS if c in want]
    assert len(got) == 1 + len(names), (tag, len(got), names)
    assert tuple(got[0]) == tuple(want["counts"]), (tag, got[0], want["counts"])
    for name, g in zip(names, got[1:]):
        w = want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (tag, name, np.nonzero(g != w)[0][:8], g[g != w][:8], w[g != w][:8])


# ---- the shared scenarios: (steps that make the map, [(cloud, R, t)] to ask it) -----------------------------------------------------
# steps: ("fold", points, R, t) | ("prune", center, radius) | ("clear", points, R, t, origin) | ("wipe",)
CLOUD_SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 127, 129, 257, 1025]  # around 32 lanes per point, 64 points per wavefront, 256 per block
MAP_POSE = E.random_pose(77)


def into_cloud_frame(targets, R, t):
    return (np.asarray(targets) - t) @ R


def dense_map():
    """about 300 rows, dense enough that most voxels have occupied neighbours"""
    return [("fold", E.gaussian(520, 7, scale=1.3), *E.IDENTITY)]


def sized_cloud(n):
    """n points around dense_map's rows, some beyond them, seen through MAP_POSE"""
    return into_cloud_frame(E.gaussian(n, 100 + n, scale=1.7), *MAP_POSE)


def faces():
    """points exactly on voxel faces, negative coordinates, -1e-20, the two ends of the key range, and points with no key at all"""
    edge = E.range_edge(VOXEL)
    e = E.CELL * VOXEL
    corners = np.array([[np.nextafter(e, 0.0)] * 3, [-e] * 3, [np.nextafter(e, 0.0), -e, 0.25], [-e, np.nextafter(e, 0.0) - 0.5, -e + 0.5]])
    tiny = np.array([[-1e-20, 0.25, 0.25], [1e-20, -1e-20, 0.0], [-0.0, 0.0, -0.0], [0.5, -0.5, 1.0], [-0.25, -0.25, -0.25]])
    rows = np.concatenate([E.on_faces(160, 3), edge, corners, tiny])
    ask = np.concatenate([E.on_faces(200, 4), edge, corners, corners + np.array([-0.3, 0.3, 0.0]), tiny,
                          E.with_nonfinite(E.on_faces(40, 5), 6), np.array([[e + 10.0, 0.0, 0.0], [0.0, -e - 10.0, 0.0], [1e300, 0.0, 0.0]])])
    return [("fold", rows, *E.IDENTITY)], [(ask, *E.IDENTITY)]


def winners(swap=False):
    """rows 0 / 1: the own voxel's row is farther than the neighbour's; row 2: only a neighbour voxel is occupied; rows 3 / 4: two
    rows exactly equidistant from the point (float32 coordinates) — swap: folded in the other order"""
    pair = np.array([[10.25, 0.25, 0.25], [10.75, 0.25, 0.25]])
    rows = np.concatenate([np.array([[0.05, 0.25, 0.25], [0.55, 0.25, 0.25], [5.25, 5.25, 5.25]]), pair[::-1] if swap else pair])
    ask = np.array([[0.45, 0.25, 0.25], [5.75, 5.25, 5.25], [10.5, 0.25, 0.25]])
    return [("fold", rows, *E.IDENTITY)], [(ask, *E.IDENTITY)]


def moved():
    """two growths (from a block of 64 rows), a prune and a ray clearing: rows move, the slot-to-row array must follow"""
    R, t = MAP_POSE
    a, b, c = E.gaussian(200, 11, scale=1.2), E.gaussian(300, 12, scale=1.6), E.gaussian(400, 13, scale=2.0)
    origin = np.array([0.1, -0.2, 0.3])
    rays = origin + (b[::3] - origin) * 1.7
    steps = [("fold", a, *E.IDENTITY), ("fold", into_cloud_frame(b, R, t), R, t), ("fold", c, *E.IDENTITY), ("prune", np.array([0.3, 0.2, -0.1]), 2.6),
             ("clear", rays, *E.IDENTITY, origin), ("fold", E.gaussian(150, 14, scale=1.5), *E.IDENTITY)]
    return steps, [(into_cloud_frame(E.gaussian(513, 15, scale=2.0), R, t), R, t), (a, *E.IDENTITY)]


def wiped():
    steps, asks = moved()
    return steps + [("wipe",)], asks


def wrapping():
    """map_evidence_ref.wrapping_cloud: 32 keys that make a table of 128 slots wrap (a map made with 64 rows and no room to grow)"""
    import map_evidence_ref as Ev

    pts = Ev.wrapping_cloud(32, 128)
    ask = np.concatenate([pts + np.array([0.1, -0.1, 0.2]), pts + np.array([0.6, 0.0, 0.0]), pts[::-1] - np.array([0.0, 0.45, 0.0])])
    return [("fold", pts, *E.IDENTITY)], [(ask, *E.IDENTITY)]


def one_voxel(n=4096):
    """n points in one voxel, folded and asked: one row, one table slot, every lane on it"""
    pts = np.array([10.25, 10.25, 5.25]) + np.random.default_rng(5).uniform(-0.2, 0.2, size=(n, 3))
    return [("fold", pts, *E.IDENTITY)], [(pts, *E.IDENTITY)]


def named(name):
    if name.startswith("size-"):
        return dense_map(), [(sized_cloud(int(name[5:])), *MAP_POSE)]
    return {"faces": faces, "winners": winners, "winners-swapped": lambda: winners(True), "moved": moved, "wiped": wiped,
            "wrapping": wrapping, "one_voxel": one_voxel}[name]()


SIZE_NAMES = ["size-%d" % n for n in CLOUD_SIZES]
OTHER_NAMES = ["faces", "winners", "winners-swapped", "moved", "wiped", "wrapping", "one_voxel"]


def same_rows_on_every_kind(steps):
    """a clearing on an evidence map weakens rows before it removes them: behind one, its rows are not the plain map's"""
    return all(s[0] != "clear" for s in steps)


def build(impl, steps):
    """runs the steps that make a map through impl: insert(points, R, t, words), prune(center, radius), clear_rays(points, R, t,
    origin), wipe() — a fold's points carry index + 1 as attribute word"""
    for s in steps:
        if s[0] == "fold":
            impl.insert(s[1], s[2], s[3], np.arange(1, s[1].shape[0] + 1, dtype=np.uint32))
        elif s[0] == "prune":
            impl.prune(s[1], s[2])
        elif s[0] == "clear":
            impl.clear_rays(s[1], s[2], s[3], s[4])
        else:
            impl.wipe()


def hold(impl, asks, tag, reaches=(0, 1), max_dist=0.3, voxel=VOXEL):
    """every question of `asks` at both reaches: impl.query(cloud, R, t, reach, max_dist, ...) with every column impl.columns()
    names against the restatement over impl's own stored rows, then the scoring form's counts; returns the expectations"""
    rows, keys = impl.rows(), impl.keys()
    attr, ev = impl.words(), impl.evidence()  # (None: the map has no such column)
    out = []
    for k, (cloud, R, t) in enumerate(asks):
        for reach in reaches:
            want = query(rows, keys, cloud, R, t, voxel, reach, max_dist, attr, ev)
            got = impl.query(cloud, R, t, reach, max_dist, True, True, attr is not None, ev is not None)
            same(got, want, (tag, k, reach))
            assert tuple(impl.query(cloud, R, t, reach, max_dist, False)) == want["counts"], (tag, k, reach, "scoring form")
            out.append(want)
    return out
