"""The host twin's merge of saved rows (madicp_host_map_merge_rows, csrc/host/voxel_map.h: VoxelMap::merge_rows) against the
restatement (tests/map_merge_ref.py) in every column after every step, on all six kinds of map; a map restored from its own
columns, which every download and every later operation cannot tell from the original; and moments of two maps that add.  The
scenarios are functions of a map factory: tests/test_gpu_map_merge.py runs the same ones on the device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cloud_export_ref as E
import map_merge_ref as G
from mad_icp_amd import capi
from map_impls import maps  # noqa: F401 (maps is a fixture)

KIND_NAMES = list(G.KINDS)


@pytest.fixture
def twin(maps):
    return lambda kind="plain", **k: maps.host(**{"voxel": G.VOXEL, "insert_attr": True, **G.KINDS[kind], **k})


def points_in(cell, count, seed):
    """`count` points strictly inside voxel `cell` under the identity"""
    u = np.random.default_rng(seed).uniform(0.05, 0.95, size=(count, 3))
    return (np.asarray(cell, np.float64) + u) * G.VOXEL


# ---- scenarios: each drives one map and returns what it saw, for a caller that compares two implementations --------------------------
def run_sized(make, kind, n):
    m = make(kind, initial_rows=1)  # (growth happens inside a merge)
    seen = [G.hold(m, G.KINDS[kind], b, (kind, n, i)) for i, b in enumerate(G.sized(G.KINDS[kind], n, 100 + n))]
    assert m.size() >= min(n, 2)
    return seen


def run_one_key(make, kind, n):
    m = make(kind, initial_rows=1)
    seen = [G.hold(m, G.KINDS[kind], b, (kind, n, i)) for i, b in enumerate(G.one_key(G.KINDS[kind], n, 7))]
    assert m.size() == 1
    if G.KINDS[kind].get("evidence"):
        assert seen[-1]["evidence"].tolist() == [G.CAP]  # (n entries of at least 1: saturated, for n >= cap)
    return seen


def run_straddling(make, kind):
    seen = []
    for i, b in enumerate(G.straddling(G.KINDS[kind], 31)):
        m = make(kind)
        seen.append(G.hold(m, G.KINDS[kind], b, (kind, i)))
        assert m.size() == 2100 - len({j for _, j in G.STRADDLES})  # (every follower gave its own key up)
    # the same key set both ways, and not the same owners: the rows of a shared key differ
    assert sorted(seen[0]["keys"].tolist()) == sorted(seen[1]["keys"].tolist()) and seen[0]["xyz"].tobytes() != seen[1]["xyz"][::-1].tobytes()
    return seen


def run_half_present(make, kind):
    """a map that real folds made, then a batch whose keys are half the map's and half new, interleaved; then its own columns again"""
    spec = G.KINDS[kind]
    m = make(kind, initial_rows=1)
    cloud = E.gaussian(1500, 5, scale=2.0)
    m.insert(cloud, *E.IDENTITY, np.arange(1500, dtype=np.uint32))
    m.insert(cloud[:700] + 0.01, *E.IDENTITY, np.arange(700, dtype=np.uint32))
    held = G.columns(m)["keys"]
    assert held.shape[0] > 600
    k = np.empty(1200, np.uint64)
    k[0::2] = held[np.random.default_rng(1).permutation(held.shape[0])[:600]]
    k[1::2] = G.distinct_keys(600, 9)
    seen = [G.hold(m, spec, G.entries(spec, k, 11), kind)]
    assert m.size() >= held.shape[0] + 590
    own = G.columns(m)
    seen.append(G.hold(m, spec, dict(own), (kind, "its own columns")))  # every key present: no row added
    assert m.size() == own["keys"].shape[0]
    return seen


def run_saturating(make, kind):
    spec = G.KINDS[kind]
    m = make(kind)
    k = G.distinct_keys(4, 3)
    b = G.entries(spec, k[[0, 1, 1, 2, 2, 2, 3]], 4, max_points=1)
    b["evidence"][:] = [1, 2, 3, 2, 2, 2, G.U31]  # 1 | 5 | 6 = cap exactly | far past it
    after = G.hold(m, spec, b, kind)
    assert after["evidence"].tolist() == [1, 5, G.CAP, G.CAP]
    b2 = G.entries(spec, k[[0, 0, 1, 3]], 5, max_points=1)
    b2["evidence"][:] = [2, 2, G.U31, 1]
    after = G.hold(m, spec, b2, kind)
    assert after["evidence"].tolist() == [5, G.CAP, G.CAP, G.CAP]
    return [after]


def run_freezes(make, kind):
    """a row already frozen takes nothing; a row the merge closes, and the next fold skips it; a new row born at n >= max_count"""
    spec = G.KINDS[kind]
    m = make(kind)
    A, B, Cn, D = (3, -2, 5), (-7, 1, 0), (10, 10, 10), (-1, -1, -1)
    kA, kB, kC, kD = (int(v) for v in G.key_of([A, B, Cn, D]))
    first = np.concatenate([points_in(A, 5, 1), points_in(B, 2, 2)])
    m.insert(first, *E.IDENTITY, np.arange(7, dtype=np.uint32))
    cols = G.columns(m)
    assert cols["keys"].tolist() == [kA, kB] and cols["moments"][:, 0].tolist() == [5, 2]
    b = G.entries(spec, np.array([kA, kB, kC, kA], np.uint64), 6, max_points=1)
    for i, c in enumerate([1, 3, 7, 2]):  # (scaled sums of one point are sums of c points at the same offset)
        b["moments"][i] *= np.uint64(c)
    seen = [G.hold(m, spec, b, kind)]
    assert seen[0]["moments"][:, 0].tolist() == [5, 5, 7]
    assert seen[0]["moments"][0].tobytes() == cols["moments"][0].tobytes()  # frozen before the merge: not a word
    again = np.concatenate([points_in(A, 3, 3), points_in(B, 3, 4), points_in(Cn, 3, 5), points_in(D, 3, 6)])
    assert m.insert(again, *E.IDENTITY, np.arange(12, dtype=np.uint32)) == (1, 4)
    after = G.columns(m)
    assert after["keys"].tolist() == [kA, kB, kC, kD] and after["moments"][:, 0].tolist() == [5, 5, 7, 3]
    assert after["moments"][:3].tobytes() == seen[0]["moments"].tobytes()  # closed by the merge, born closed: the fold skips them
    assert after["evidence"].tolist() == [min(int(e) + 2, G.CAP) for e in seen[0]["evidence"]] + [2]  # (the hits still count)
    seen.append(after)
    seen.append(G.hold(m, spec, G.entries(spec, np.array([kB, kC, kD, kD], np.uint64), 8), kind))
    assert seen[-1]["moments"][:3].tobytes() == after["moments"][:3].tobytes() and seen[-1]["moments"][3, 0] > 3
    return seen


def run_odd_bits(make, kind):
    spec = G.KINDS[kind]
    m = make(kind)
    b = G.odd_bits(spec, 21)
    after = G.hold(m, spec, b, kind)
    assert after["xyz"].view(np.uint32).tobytes() == b["xyz"].view(np.uint32).tobytes() and np.isnan(after["xyz"]).sum() >= 9
    if after["attr"] is not None:
        assert after["attr"].tobytes() == b["attr"].tobytes()
    return [after, G.hold(m, spec, G.take(b, np.arange(8)[::-1]), kind)]  # (all present: nothing of xyz and attr changes)


def run_edges(make, kind):
    spec = G.KINDS[kind]
    m = make(kind)
    m.insert(points_in((0, 0, 0), 1, 1), *E.IDENTITY, np.zeros(1, np.uint32))
    held = G.columns(m)["keys"][0]
    seen = [G.hold(m, spec, G.entries(spec, np.zeros(0, np.uint64), 1), (kind, "n = 0"))]
    assert G.call(m, dict(keys=np.zeros(0, np.uint64), xyz=np.zeros((0, 3), np.float32), attr=None, evidence=None, moments=None)) == (0, 1)
    seen.append(G.hold(m, spec, G.legal_edges(spec, held), (kind, "legal edges")))
    return seen


SCENARIOS = {"straddling": run_straddling, "half_present": run_half_present, "odd_bits": run_odd_bits, "edges": run_edges}


@pytest.mark.parametrize("n", G.SIZES)
def test_host_merge_is_the_restatement_at_every_size(twin, n):
    for kind in KIND_NAMES:
        run_sized(twin, kind, n)


@pytest.mark.parametrize("n", [1025, 4097])
def test_host_merge_of_n_entries_on_one_key(twin, n):
    for kind in KIND_NAMES:
        run_one_key(twin, kind, n)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_host_merge_scenarios(twin, name):
    for kind in KIND_NAMES:
        SCENARIOS[name](twin, kind)


def test_host_merge_evidence_saturates(twin):
    for kind in ("ev", "attr_ev", "ev_mom", "attr_ev_mom"):
        run_saturating(twin, kind)


def test_host_merge_and_the_freeze(twin):
    for kind in ("ev_mom", "attr_ev_mom"):
        run_freezes(twin, kind)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def raw_args(b, n=None):
    p = lambda a, ct: None if a is None else np.ascontiguousarray(a).ctypes.data_as(ct)
    u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    return (p(b["keys"], u64), p(b["xyz"], C.POINTER(C.c_float)), p(b["attr"], u32), p(b["evidence"], u32), p(b["moments"], u64),
            b["keys"].shape[0] if n is None else n)


def run_refusals(make, kind, raw):
    """raw(m, voxel, batch, n=None, answers=True, handle=True) -> (rc, added, rows): every refusal leaves every column and both
    answers as they were"""
    spec = G.KINDS[kind]
    m = make(kind, max_rows=12)
    m.insert(np.concatenate([points_in((0, 0, 0), 2, 1), points_in((4, 0, -3), 1, 2)]), *E.IDENTITY, np.arange(3, dtype=np.uint32))
    before = G.columns(m)
    assert before["keys"].shape[0] == 2
    cases = G.refusal_cases(spec, before["keys"][1])
    assert len(cases) >= 8
    for label, b, voxel in cases:
        want = G.refusal(before, b, spec, voxel, max_rows=12)
        assert want == G.INVALID, label
        assert raw(m, voxel, b) == (G.INVALID, -7, -7), (kind, label)
        G.same(G.columns(m), before)
    good = cases[0][1]
    assert raw(m, G.VOXEL, good, n=-1) == (G.INVALID, -7, -7) and raw(m, G.VOXEL, good, n=(1 << 30) + 1) == (G.INVALID, -7, -7)
    assert raw(m, G.VOXEL, good, answers=False)[0] == G.INVALID and raw(m, G.VOXEL, good, handle=False)[0] == G.INVALID
    missing = dict(good)
    missing["xyz"] = None
    assert raw(m, G.VOXEL, missing) == (G.INVALID, -7, -7)
    eleven = G.entries(spec, np.tile(before["keys"], 6)[:11], 3, max_points=1)  # rows + n > max_rows, though no row would be added
    assert G.refusal(before, eleven, spec, G.VOXEL, max_rows=12) == G.CAPACITY
    assert raw(m, G.VOXEL, eleven) == (G.CAPACITY, -7, -7)
    G.same(G.columns(m), before)
    assert G.refusal(before, good, spec, G.VOXEL, max_rows=12) is None and raw(m, G.VOXEL, good) == (0, 4, 6)  # (and the good one goes in)
    return G.columns(m)


def host_raw(m, voxel, b, n=None, answers=True, handle=True):
    added, rows = C.c_int64(-7), C.c_int64(-7)
    rc = capi.host_lib().madicp_host_map_merge_rows(m.h if handle else None, float(voxel), *raw_args(b, n), C.byref(added) if answers else None,
                                                    C.byref(rows) if answers else None)
    return rc, added.value, rows.value


def test_host_merge_refusals_leave_everything(twin):
    for kind in KIND_NAMES:
        run_refusals(twin, kind, host_raw)


# ---- a map restored from its own columns ----------------------------------------------------------------------------------------
def everything(m):
    """every download of a map, as bytes"""
    out = [c.tobytes() for c in G.columns(m).values() if c is not None] + [m.rows(5).tobytes() if m.size() > 5 else b""]
    if m.params is not None:
        out += [c.tobytes() for c in m.confirmed(3)]
    if m.max_count is not None:
        out += [c.tobytes() for c in m.surfels()]
    return out


def run_round_trip(make, kind):
    """map A from three clouds of about 2 000 points with a clearing and a prune between them; B = A's columns merged into a fresh
    map of the same spec; then both driven alike.  Returns everything either answered, for a caller with two implementations."""
    spec = G.KINDS[kind]
    clouds = [E.gaussian(2000, 40 + i, scale=2.5) + np.array([0.6 * i, 0.0, 0.0]) for i in range(5)]
    words = [np.random.default_rng(50 + i).integers(0, 1 << 32, size=2000, dtype=np.uint64).astype(np.uint32) for i in range(5)]
    origin = np.array([0.05, -0.1, 0.02])
    a, b = make(kind, initial_rows=512), make(kind, initial_rows=1)
    a.insert(clouds[0], *E.IDENTITY, words[0])
    cleared = [a.clear_rays(clouds[1][:600] * 1.5, *E.IDENTITY, origin)[0] for _ in range(2)]  # (evidence 2, miss 1: the second one removes)
    assert cleared[1] > 0 or (not spec.get("evidence") and cleared[0] > 0)
    a.insert(clouds[1], *E.IDENTITY, words[1])
    assert a.prune(np.array([0.3, 0.0, 0.0]), 5.0)[0] > 0
    a.insert(clouds[2], *E.IDENTITY, words[2])
    saved = G.columns(a)
    assert G.call(b, saved) == (a.size(), a.size()) and a.size() > 1500
    assert everything(b) == everything(a)
    R, t = E.random_pose(3)
    t = t * 0.05
    seen = []
    poses = np.stack([np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), np.concatenate([R.reshape(-1), t])])
    for m in (a, b):
        m.track(True)
    for m in (a, b):
        got = dict(folds=[m.insert(clouds[3], *E.IDENTITY, words[3]), m.insert(clouds[4], R, t, words[4])])
        got["clearing"] = m.clear_rays(clouds[2][:500] * 1.4, *E.IDENTITY, origin, 0.1, m.size() - 100)
        got["prune"] = m.prune(np.array([1.0, 0.0, 0.0]), 4.5, got["clearing"][2])
        got["log"] = [c.tobytes() for c in m.take()]
        got["query"] = [np.asarray(c).tobytes()
                        for c in m.query(clouds[0][:700], R, t, 1, 0.3, True, True, spec.get("with_attr", False), bool(spec.get("evidence")))]
        got["score"] = m.map.score(*scan_of(m, clouds[1][:800]), poses, 1, 0.3, 3).tobytes()
        got["columns"] = G.columns(m)
        if m.max_count is not None:  # (eigenvalues and normals go through the side's own trigonometry: equal on ONE side only)
            r = m.register(clouds[2][:900], R, t, 2, max_dist=0.4)
            got["register"] = [r[k].tobytes() for k in ("R", "t", "X", "H", "b", "chi2", "counts")]
        got["everything"] = everything(m)
        seen.append(got)
    assert seen[0]["prune"][0] > 0 and len(seen[0]["log"][0]) > 0 and seen[0]["folds"][1][0] > 0  # (rows left, the log holds some)
    for name in seen[0]:
        if name == "columns":
            G.same(seen[0][name], seen[1][name])
        else:
            assert seen[0][name] == seen[1][name], (kind, name)
    return seen[0]


def scan_of(m, cloud):
    """what _Map.score takes as its scan: the points on the host; on the device a cloud the map keeps until it is closed"""
    if hasattr(m, "ctx"):
        key = ("score", cloud.shape[0])
        if key not in m.clouds:
            m.clouds[key] = m.cloud(cloud)
        return (m.clouds[key],)
    return (cloud,)


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_host_map_restored_from_its_columns_is_the_map(twin, kind):
    run_round_trip(twin, kind)


# ---- moments of two maps add ----------------------------------------------------------------------------------------------------
def run_additivity(make):
    """no evidence, max_count = 2^31 (nothing ever freezes): the rows of map(X) merged into map(Y) against a map folded from both"""
    spec = dict(max_count=1 << 31)
    X = [E.gaussian(2000, 60, scale=2.0), E.gaussian(1500, 61, scale=2.0) + 0.3]
    Y = [E.gaussian(2000, 62, scale=2.0) + np.array([0.5, 0.0, 0.0]), E.gaussian(1800, 63, scale=2.0)]
    mx, my, both = (make("plain", **spec) for _ in range(3))
    for c in X:
        mx.insert(c, *E.IDENTITY, None)
    for c in Y:
        my.insert(c, *E.IDENTITY, None)
    for c in X + Y:
        both.insert(c, *E.IDENTITY, None)
    G.hold(my, spec, G.columns(mx), "X's rows into map(Y)")
    got, want = G.columns(my), G.columns(both)
    by_key = lambda c: {int(k): row.tobytes() for k, row in zip(c["keys"], c["moments"])}
    assert by_key(got) == by_key(want) and len(by_key(got)) == got["keys"].shape[0] > 3000
    assert int(got["moments"][:, 0].sum()) == 7300
    # row order and xyz may differ, and here they do: `both` folded X first, so a voxel that X and Y share holds X's first point
    # there and Y's in the merged map, and X's new rows stand behind all of Y's
    assert got["keys"].tobytes() != want["keys"].tobytes() and got["xyz"].tobytes() != want["xyz"].tobytes()
    return got


def test_host_moments_of_two_maps_add(twin):
    run_additivity(twin)
