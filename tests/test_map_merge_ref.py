"""The restatement of the merge rule (tests/map_merge_ref.py) held to what section 1 of the rule says in words — on small cases
worked out by hand, and on properties the rule promises: the order of a batch's entries decides the rows' order and owners and
nothing else, a batch split in two merges gives the same evidence (saturating addition commutes) and, while nothing freezes, the
same moments; what the header states as constants is what the restatement and the tests stand on.  No library is loaded."""
import os
import re

import numpy as np

import map_merge_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = dict(with_attr=True, evidence=G.EVIDENCE, max_count=G.MAX_COUNT)


def test_the_headers_constants_are_the_restatements():
    merge = open(os.path.join(ROOT, "mad_icp_amd", "csrc", "common", "map_merge.h")).read()
    moments = open(os.path.join(ROOT, "mad_icp_amd", "csrc", "common", "voxel_moments.h")).read()
    assert int(re.search(r"kMergeEvidenceMax = (0x[0-9a-f]+)u;", merge).group(1), 16) == G.U31
    assert int(re.search(r"kMergeCountMax = (0x[0-9a-f]+)ull;", merge).group(1), 16) == G.U31
    assert int(re.search(r"kMergeOffsetMax = (\d+)ull;", merge).group(1)) == 65535
    assert int(re.search(r"kMomentWords = (\d+);", moments).group(1)) == 10
    scan = open(os.path.join(ROOT, "mad_icp_amd", "csrc", "hip", "tree_build.hip.h")).read()
    assert int(re.search(r"constexpr int kScanTile = (\d+);", scan).group(1)) == 1024 and {63, 64, 65, 1023, 1024, 1025} <= set(G.SIZES)


def test_a_case_worked_out_by_hand():
    k = G.key_of([(0, 0, 0), (1, 0, 0), (-1, -1, -1), (5, 5, 5)])
    assert k[0] == (1 << 20) | (1 << 41) | (1 << 62) and k[2] == ((1 << 20) - 1) * (1 | (1 << 21) | (1 << 42))
    cols = dict(keys=k[:2].copy(), xyz=np.array([[1, 2, 3], [4, 5, 6]], np.float32), attr=np.array([10, 11], np.uint32),
                evidence=np.array([5, 1], np.uint32), moments=np.array([[4, 1, 1, 1, 1, 1, 1, 1, 1, 1], [3, 2, 2, 2, 2, 2, 2, 2, 2, 2]], np.uint64))
    batch = dict(keys=k[[3, 1, 2, 0, 2, 1]], xyz=np.arange(18, dtype=np.float32).reshape(6, 3) + 100, attr=np.arange(6, dtype=np.uint32) + 50,
                 evidence=np.array([7, 1, 2, 3, 2, 2], np.uint32), moments=np.tile(np.array([2, 9, 9, 9, 40, 40, 40, 40, 40, 40], np.uint64), (6, 1)))
    out, added = G.merge(cols, batch, SPEC)
    assert added == 2 and out["keys"].tolist() == [int(k[0]), int(k[1]), int(k[3]), int(k[2])]  # (5, 5, 5) came first, at index 0
    assert out["xyz"].tolist() == [[1, 2, 3], [4, 5, 6], [100, 101, 102], [106, 107, 108]]  # new rows: their LOWEST entry's floats
    assert out["attr"].tolist() == [10, 11, 50, 52]
    assert out["evidence"].tolist() == [6, 4, 6, 4]  # min(5 + 3, 6) | 1 + 1 + 2 | min(7, 6) | 2 + 2
    # row 0 held n = 4 = max_count: frozen, not a word; row 1 (n = 3 < 4) takes BOTH its entries, though the first brings it past 4
    assert out["moments"].tolist() == [[4] + [1] * 9, [7] + [20] * 3 + [82] * 6, [2] + [9] * 3 + [40] * 6, [4] + [18] * 3 + [80] * 6]
    again, added = G.merge(out, batch, SPEC)  # only the row of (5, 5, 5), n = 2, is still below max_count; evidence saturates on
    assert added == 0 and again["moments"][[0, 1, 3]].tobytes() == out["moments"][[0, 1, 3]].tobytes()
    assert again["moments"][2].tolist() == [4] + [18] * 3 + [80] * 6 and again["evidence"].tolist() == [6, 6, 6, 6]
    assert again["xyz"].tobytes() == out["xyz"].tobytes() and again["attr"].tobytes() == out["attr"].tobytes()


def test_the_order_of_entries_decides_rows_and_owners_only():
    spec = dict(with_attr=True, evidence=G.EVIDENCE, max_count=1 << 31)
    keys = G.distinct_keys(40, 1)[np.random.default_rng(2).integers(0, 40, size=300)]
    b = G.entries(spec, keys, 3)
    start = G.merge(G.empty(spec), G.entries(spec, G.distinct_keys(40, 1)[:15], 4), spec)[0]
    a, _ = G.merge(start, b, spec)
    c, _ = G.merge(start, G.take(b, np.random.default_rng(5).permutation(300)), spec)
    by_key = lambda cols, name: {int(k): v.tobytes() for k, v in zip(cols["keys"], cols[name])}
    assert by_key(a, "evidence") == by_key(c, "evidence") and by_key(a, "moments") == by_key(c, "moments")
    assert a["keys"][:15].tobytes() == c["keys"][:15].tobytes() == start["keys"].tobytes() and a["keys"].tobytes() != c["keys"].tobytes()
    assert a["xyz"][:15].tobytes() == c["xyz"][:15].tobytes() == start["xyz"].tobytes()


def test_a_batch_in_two_merges():
    keys = G.distinct_keys(30, 7)[np.random.default_rng(8).integers(0, 30, size=200)]
    for max_count, moments_equal in ((1 << 31, True), (G.MAX_COUNT, False)):
        spec = dict(evidence=G.EVIDENCE, max_count=max_count)
        b = G.entries(spec, keys, 9)
        once, _ = G.merge(G.empty(spec), b, spec)
        half, _ = G.merge(G.empty(spec), G.take(b, np.arange(100)), spec)
        twice, _ = G.merge(half, G.take(b, np.arange(100, 200)), spec)
        assert once["keys"].tobytes() == twice["keys"].tobytes() and once["xyz"].tobytes() == twice["xyz"].tobytes()
        assert once["evidence"].tobytes() == twice["evidence"].tobytes()
        # one merge is one fold: a row takes all of it or none — two merges let a row freeze in between
        assert (once["moments"].tobytes() == twice["moments"].tobytes()) == moments_equal
        assert (twice["moments"][:, 0] <= once["moments"][:, 0]).all()


def test_refusals_of_the_restatement():
    spec = SPEC
    cols = G.merge(G.empty(spec), G.entries(spec, G.distinct_keys(3, 1), 2), spec)[0]
    cases = G.refusal_cases(spec, cols["keys"][1])
    assert all(G.refusal(cols, b, spec, voxel) == G.INVALID for _, b, voxel in cases), [c[0] for c in cases]
    assert {"voxel", "attr missing", "evidence missing", "moments missing", "bit 63", "evidence 0", "count 0", "S1", "S2", "total"} <= {c[0] for c in cases}
    plain = G.refusal_cases({}, cols["keys"][1])
    assert {"attr surplus", "evidence surplus", "moments surplus"} <= {c[0] for c in plain}
    good = G.entries(spec, G.distinct_keys(5, 3), 4)
    assert G.refusal(cols, good, spec, G.VOXEL) is None and G.refusal(cols, good, spec, G.VOXEL, max_rows=7) == G.CAPACITY
    assert G.refusal(cols, good, spec, G.VOXEL, max_rows=8) is None
    assert G.refusal(cols, G.legal_edges(spec, cols["keys"][0]), spec, G.VOXEL) is None
    assert G.refusal(cols, G.empty(spec), spec, G.VOXEL) is None and G.refusal(cols, G.empty({}), spec, G.VOXEL) is None  # n == 0
