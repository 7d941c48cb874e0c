"""A numpy / Python-integer restatement of the merge rule (csrc/common/map_merge.h; include/madicp_hip.h: madicp_map_merge_rows),
and the cases the host twin (tests/test_host_map_merge.py) and the device (tests/test_gpu_map_merge.py) are held to.

A map is its columns — keys (M,) uint64, xyz (M, 3) float32, attr / evidence (M,) uint32, moments (M, 10) uint64, None where the map
has no such column — and merge() is a function of (columns, batch) alone: which rows are new and where they go, what their words
become.  It needs no freeze word: between two folds a row is frozen iff its count is >= max_count.  Sums are Python integers.
Floats and attribute words are never looked at as values: everything is compared as bytes."""
import numpy as np

VOXEL = 0.25
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4097]  # one past a wavefront (64) and past a 1024-entry scan tile
CAP, MAX_COUNT = 6, 4
EVIDENCE = (2, 1, CAP)
# the six kinds: plain / attribute x none / evidence / evidence + moments — as what tests/map_impls.py's adapters take
KINDS = {
    "plain": dict(), "attr": dict(with_attr=True),
    "ev": dict(evidence=EVIDENCE), "attr_ev": dict(with_attr=True, evidence=EVIDENCE),
    "ev_mom": dict(evidence=EVIDENCE, max_count=MAX_COUNT), "attr_ev_mom": dict(with_attr=True, evidence=EVIDENCE, max_count=MAX_COUNT),
}
INVALID, CAPACITY = -1, -4
U31 = (1 << 31) - 1


def key_of(cells):
    """export_key's packing of integer cells (n, 3), each in [-2^20, 2^20)"""
    c = np.asarray(cells, np.int64).reshape(-1, 3) + (1 << 20)
    return (c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)).astype(np.uint64)


def distinct_keys(n, seed):
    """n distinct keys, in a random order, of cells within +-2^19 (negative ones included)"""
    rng = np.random.default_rng(seed)
    cells = np.unique(rng.integers(-(1 << 19), 1 << 19, size=(2 * n + 8, 3)), axis=0)
    return key_of(cells[rng.permutation(cells.shape[0])[:n]])


def entries(spec, keys, seed, max_points=3, max_e=3):
    """a batch for a map of `spec` on the given keys: arbitrary float bits, arbitrary words, evidence 1 .. max_e, and moments that
    are the sums of 1 .. max_points points of 16-bit offsets (so every entry is one a map could hand out)"""
    rng = np.random.default_rng(seed)
    keys = np.ascontiguousarray(keys, np.uint64)
    n = keys.shape[0]
    b = dict(keys=keys, xyz=rng.normal(size=(n, 3)).astype(np.float32) * 7, attr=None, evidence=None, moments=None)
    if spec.get("with_attr"):
        b["attr"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if spec.get("evidence"):
        b["evidence"] = rng.integers(1, max_e + 1, size=n).astype(np.uint32)
    if spec.get("max_count"):
        M = np.zeros((n, 10), np.uint64)
        cnt = rng.integers(1, max_points + 1, size=n)
        for p in range(max_points):
            w = rng.integers(0, 65536, size=(n, 3)).astype(np.uint64) * (cnt > p)[:, None].astype(np.uint64)
            M[:, 1:4] += w
            M[:, 4] += w[:, 0] * w[:, 0]
            M[:, 5] += w[:, 0] * w[:, 1]
            M[:, 6] += w[:, 0] * w[:, 2]
            M[:, 7] += w[:, 1] * w[:, 1]
            M[:, 8] += w[:, 1] * w[:, 2]
            M[:, 9] += w[:, 2] * w[:, 2]
        M[:, 0] = cnt
        b["moments"] = M
    return b


def take(batch, index):
    return {k: (None if v is None else np.ascontiguousarray(v[index])) for k, v in batch.items()}


def empty(spec):
    return dict(keys=np.zeros(0, np.uint64), xyz=np.zeros((0, 3), np.float32), attr=np.zeros(0, np.uint32) if spec.get("with_attr") else None,
                evidence=np.zeros(0, np.uint32) if spec.get("evidence") else None,
                moments=np.zeros((0, 10), np.uint64) if spec.get("max_count") else None)


def merge(cols, batch, spec):
    """(columns after the merge, rows added)"""
    cap = spec["evidence"][2] if spec.get("evidence") else None
    max_count = spec.get("max_count")
    keys = [int(k) for k in cols["keys"]]
    row_of = {k: j for j, k in enumerate(keys)}
    bkeys = [int(k) for k in batch["keys"]]
    first = {}
    for i, k in enumerate(bkeys):
        first.setdefault(k, i)  # (insertion order: ascending lowest index)
    new = [k for k in first if k not in row_of]
    owner = [first[k] for k in new]
    for k in new:
        row_of[k] = len(keys)
        keys.append(k)
    out = dict(keys=np.array(keys, np.uint64), xyz=np.concatenate([cols["xyz"].view(np.uint32), batch["xyz"].view(np.uint32)[owner]]).view(np.float32),
               attr=None, evidence=None, moments=None)
    if cols["attr"] is not None:
        out["attr"] = np.concatenate([cols["attr"], batch["attr"][owner]]).astype(np.uint32)
    if cap is not None:
        e = [int(v) for v in cols["evidence"]] + [0] * len(new)
        s = [0] * len(keys)
        for k, v in zip(bkeys, batch["evidence"]):
            s[row_of[k]] += int(v)
        out["evidence"] = np.array([min(a + b, cap) if b else a for a, b in zip(e, s)], np.uint32)
    if max_count is not None:
        M = [[int(v) for v in row] for row in cols["moments"]] + [[0] * 10 for _ in new]
        before = [row[0] for row in M]
        for k, E in zip(bkeys, batch["moments"]):
            r = row_of[k]
            if before[r] < max_count:
                M[r] = [a + int(b) for a, b in zip(M[r], E)]
        assert all(v < (1 << 64) for row in M for v in row)
        out["moments"] = np.array(M, np.uint64).reshape(-1, 10)
    return out, len(new)


def refusal(cols, batch, spec, voxel, map_voxel=VOXEL, max_rows=1 << 24):
    """None, INVALID or CAPACITY: section 1's refusals, in the order of the one pass"""
    n = batch["keys"].shape[0]
    has = dict(attr=bool(spec.get("with_attr")), evidence=bool(spec.get("evidence")), moments=bool(spec.get("max_count")))
    if voxel != map_voxel:
        return INVALID
    for name, there in has.items():
        if batch[name] is not None and not there:
            return INVALID
        if batch[name] is None and there and n > 0:
            return INVALID
    if any(int(k) >> 63 for k in batch["keys"]):
        return INVALID
    if has["evidence"] and n and any(not 1 <= int(e) <= U31 for e in batch["evidence"]):
        return INVALID
    if has["moments"] and n:
        total = 0
        for row in batch["moments"]:
            c = int(row[0])
            if c < 1 or any(int(v) > 65535 * c for v in row[1:4]) or any(int(v) > 65535 * 65535 * c for v in row[4:]):
                return INVALID
            total += c
        if total > U31:
            return INVALID
    if cols["keys"].shape[0] + n > max_rows:
        return CAPACITY
    return None


def same(a, b):
    """two sets of columns, byte for byte (None where the map has no such column)"""
    assert set(a) == set(b)
    for name in a:
        if a[name] is None or b[name] is None:
            assert a[name] is None and b[name] is None, name
            continue
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, (name, a[name].dtype, b[name].dtype, a[name].shape, b[name].shape)
        assert a[name].tobytes() == b[name].tobytes(), name


def columns(m):
    """every column of a tests/map_impls.py map under the names used here"""
    c = m.columns()
    return dict(keys=c["keys"], xyz=c["xyz"], attr=c.get("attr"), evidence=c.get("evidence"), moments=c.get("moments"))


def call(m, batch, voxel=VOXEL):
    return m.map.merge_rows(voxel, batch["keys"], batch["xyz"], batch["attr"], batch["evidence"], batch["moments"])


def hold(m, spec, batch, label):
    """one merge into map m, held to the restatement in every column and both counts; returns the columns afterwards"""
    before = columns(m)
    want, added = merge(before, batch, spec)
    got = call(m, batch)
    assert got == (added, want["keys"].shape[0]), (label, got, added)
    after = columns(m)
    same(after, want)
    return after


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def sized(spec, n, seed):
    """two batches of n entries: keys drawn with repeats from a pool, then half of them again with as many unseen ones"""
    rng = np.random.default_rng(seed)
    pool = distinct_keys(max(n, 2), seed)
    k1 = pool[rng.integers(0, max((2 * n) // 3, 1), size=n)]
    k2 = np.where(rng.integers(0, 2, size=n) == 1, pool[rng.integers(0, pool.shape[0], size=n)], distinct_keys(n, seed + 1))
    return [entries(spec, k1, seed + 2), entries(spec, k2, seed + 3)]


def one_key(spec, n, seed):
    """all n entries on ONE key, twice: the row is made, then found"""
    k = np.full(n, distinct_keys(1, seed)[0], np.uint64)
    return [entries(spec, k, seed + 1, max_points=1), entries(spec, k, seed + 2, max_points=1)]


STRADDLES = [(62, 63), (63, 64), (64, 65), (0, 64), (63, 128), (1022, 1023), (1023, 1024), (1024, 1025), (5, 1024), (1023, 2047), (64, 2048)]


def straddling(spec, seed):
    """2100 entries on distinct keys, but for the pairs (i, j) of STRADDLES, which share one: the owner i and the follower j sit on
    both sides of lane 63 / 64 and of entry 1023 / 1024 — the same wavefront, the next one, a later tile.  Then the batch
    reversed, into a fresh map: every owner is now the entry that followed."""
    k = distinct_keys(2100, seed)
    for i, j in STRADDLES:
        k[j] = k[i]
    b = entries(spec, k, seed + 1)
    return b, take(b, np.arange(2100)[::-1])


NAN_BITS = np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0xff923456, 0x80000000, 0x00000000, 0x7f800000, 0x00000001], np.uint32)


def odd_bits(spec, seed):
    """rows of NaN (quiet and signalling, both signs, payloads), -0.0, +inf and a denormal; attribute words of the same bits"""
    n = NAN_BITS.shape[0]
    b = entries(spec, distinct_keys(n, seed), seed + 1)
    b["xyz"] = np.stack([NAN_BITS, np.roll(NAN_BITS, 1), np.roll(NAN_BITS, 3)], axis=1).view(np.float32).copy()
    if b["attr"] is not None:
        b["attr"] = np.roll(NAN_BITS, 2).copy()
    return b


def refusal_cases(spec, held):
    """(label, batch, voxel): every refusal of section 1 on a batch of 5 entries, one of whose keys the map holds (`held`)"""
    k = distinct_keys(5, 77)
    k[2] = held
    good = entries(spec, k, 78)
    out = [("voxel", good, VOXEL * 2), ("voxel nan", good, float("nan")), ("voxel off by an ulp", good, np.nextafter(VOXEL, 1.0))]

    def with_(name, value):
        b = dict(good)
        b[name] = value
        return b

    for name, there, surplus in (("attr", spec.get("with_attr"), np.arange(5, dtype=np.uint32)), ("evidence", spec.get("evidence"), np.ones(5, np.uint32)),
                                 ("moments", spec.get("max_count"), np.ones((5, 10), np.uint64))):
        out.append((name + (" missing" if there else " surplus"), with_(name, None if there else surplus), VOXEL))
    bad = k.copy()
    bad[4] |= np.uint64(1 << 63)
    out.append(("bit 63", with_("keys", bad), VOXEL))
    out.append(("no key", with_("keys", np.full(5, ~np.uint64(0), np.uint64)), VOXEL))
    if spec.get("evidence"):
        for v in (0, 1 << 31, (1 << 32) - 1):
            e = good["evidence"].copy()
            e[3] = v
            out.append(("evidence %d" % v, with_("evidence", e), VOXEL))
    if spec.get("max_count"):
        def mom(row, col, value):
            M = good["moments"].copy()
            M[row, col] = value
            return with_("moments", M)

        c = int(good["moments"][1, 0])
        out += [("count 0", mom(1, 0, 0), VOXEL), ("count 2^31", mom(1, 0, 1 << 31), VOXEL), ("count 2^63", mom(1, 0, 1 << 63), VOXEL),
                ("S1", mom(1, 2, 65535 * c + 1), VOXEL), ("S1 top", mom(1, 3, (1 << 64) - 1), VOXEL),
                ("S2", mom(1, 4, 65535 * 65535 * c + 1), VOXEL), ("S2 cross", mom(1, 8, 65535 * 65535 * c + 1), VOXEL)]
        M = good["moments"].copy()
        M[:, 0] = [U31 - 3, 1, 1, 1, 1]  # each legal, together 2^31
        M[:, 1:] = 0
        out.append(("total", with_("moments", M), VOXEL))
    return out


def legal_edges(spec, held):
    """what section 1 allows at its edges: evidence 2^31 - 1, sums exactly at 65535 n and 65535^2 n, counts that sum to 2^31 - 1"""
    k = distinct_keys(3, 91)
    k[1] = held
    b = entries(spec, k, 92)
    if b["evidence"] is not None:
        b["evidence"][:] = [U31, 1, U31]
    if b["moments"] is not None:
        c = U31 - 2
        b["moments"][0] = [c] + [65535 * c] * 3 + [65535 * 65535 * c] * 6
        b["moments"][1] = [1] + [0] * 9
        b["moments"][2] = [1] + [65535] * 3 + [65535 * 65535] * 6
    return b
