"""GPU tests of the device front-end: MAD-tree construction, deskew and scan ingest on the
MI355X, against the host builder (bit-identical to the oracle's, tests/test_host_builder.py), the oracle's deskew
(oracle_lib.deskew, pipeline.cpp:79-123) and a numpy restatement of bin_runner.cpp:126-166.

What "parity" means here, stated per piece:
  * ingest        — bit-identical (conversion, float-norm range filter, Eigen's AngleAxisd rotation in its own order).
  * deskew        — every output point is bit-identical to one of the oracle's output points and vice versa (the cloud as
                    a multiset), same time chunks; the ORDER of points whose azimuths tie may differ (std::sort is not
                    stable and the synthetic scans hold 64 points per azimuth column); with distinct azimuths the output
                    is the oracle's row for row.
  * tree build    — not bitwise, by construction (mad_icp_amd/csrc/hip/tree_build.hip.h: parallel sums, device
                    trigonometry) — but the same decisions and the same MEMBER ORDER as the reference's in-place split
                    (utils.h:37-52, common/split_order.h), so that "first member wins" (mad_tree.cpp:76-86) picks the host
                    builder's representative.  Measured on these inputs and asserted: identical leaf count and topology,
                    every leaf mean is an input point, on the scans and the Gaussian clouds EVERY leaf mean is the host
                    builder's at the same leaf ordinal (asserted >= 99.9 %), the construction leaves the points in the
                    host builder's order row for row (madicp_debug_tree_build_points), registrations against
                    device-built maps land within 1e-4 m of registrations against host-built maps.  What differs: the
                    last bits of centroids, split normals, leaf normals and extents (serial vs parallel sums, libm vs
                    device atan2 / cos / sin), and with them decisions that sit within rounding of their threshold
                    (equally spaced collinear points: three-point leaves whose outer members tie EXACTLY).
                    Exact properties that must hold regardless: valid DFS preorder (the validating upload accepts it),
                    leaf ordinals in getLeafs() order, a leaf mean queried against its own tree returns itself at
                    distance exactly 0 (the reference's nn_search.py property), bit-reproducible run to run, and the
                    device-made LDS-top layout equals the host-made one (identical registration results either way).
                    HOW FAR those last bits may go, and what they do to correspondences, is held elsewhere:
                    tests/test_gpu_default_path_parity.py audits every internal node of a device-built tree against its
                    members' centroid and principal axis in extended precision (what bounds the internal nodes this file
                    only counts as "bitwise equal on >= 0.6"), holds the kernels on device-built trees to a plain
                    reference of the descent exactly, and counts the decisions that differ from the oracle's.
"""
import numpy as np
import pytest

import oracle_lib as O
from fixtures import B_MAX, B_MIN, PARAMS, full_scan, street_problem
from mad_icp_amd import capi, synth

pytestmark = pytest.mark.gpu


def keyset(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return set(map(bytes, a.view(np.uint8).reshape(a.shape[0], 24)))


def build_both(ctx, pts, b_max=B_MAX, b_min=B_MIN):
    ht = capi.HostTree(pts, b_max, b_min, 2)
    cid = ctx.cloud_upload(pts)
    tid, nl = ctx.tree_build(cid, b_max, b_min)
    nn, nl2 = ctx.tree_info(tid)
    assert nl2 == nl and nn == 2 * nl - 1
    nodes = ctx.tree_download(tid, nn)
    return ht, cid, tid, nodes


def check_exact_properties(ctx, pts, tid, nodes):
    nl = (nodes.shape[0] + 1) // 2
    # a valid DFS-preorder tree: the validating upload path accepts the downloaded array
    t2 = ctx.tree_upload(nodes, nl)
    ctx.tree_release(t2)
    leaf = nodes["right"] == 0
    assert leaf.sum() == nl
    assert np.array_equal(nodes["leaf_id"][leaf], np.arange(nl))       # getLeafs() order == preorder of appearance
    assert (nodes["leaf_id"][~leaf] == -1).all()
    assert keyset(nodes["mean"][leaf]) <= keyset(pts)                   # every leaf mean is a member (mad_tree.cpp:76-86)
    r = ctx.nn_search(tid, nodes["mean"][leaf], want=("leaf", "dist"))
    finite = np.isfinite(nodes["mean"][leaf]).all(axis=1)
    assert (r["dist"][finite] == 0.0).all()
    assert np.array_equal(r["leaf"][finite], np.arange(nl)[finite])


@pytest.mark.parametrize("name", ["1pt", "2pt", "dup40", "line100", "expline36", "gauss3000", "street19k", "scan120k"])
def test_device_tree_build_vs_host_builder(mctx, name):
    ctx = mctx  # (the measurement build's context: madicp_debug_tree_build_points below)
    rng = np.random.default_rng(5)
    pts = {
        "1pt": lambda: np.array([[1.0, 2.0, 3.0]]),
        "2pt": lambda: np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]]),
        "dup40": lambda: np.repeat(np.array([[1.0, 2.0, 3.0]]), 40, axis=0),
        "line100": lambda: np.stack([np.linspace(0, 10, 100), np.zeros(100), np.zeros(100)], 1),
        # collinear points a factor 100 apart: the mean split peels one point per level — a tree 35 levels deep, past
        # the launch sequence's first 20 levels (the builder's continue-and-check loop)
        "expline36": lambda: np.stack([100.0 ** np.arange(36), np.zeros(36), np.zeros(36)], 1),
        "gauss3000": lambda: rng.normal(size=(3000, 3)) * [5, 3, 0.05],
        "street19k": lambda: street_problem(2)["query_scans"][0],
        "scan120k": lambda: synth.make_problem(1, seed=1, n_queries=1)["query_scans"][0],
    }[name]()
    ht, cid, tid, nodes = build_both(ctx, pts)
    check_exact_properties(ctx, pts, tid, nodes)
    nl = (nodes.shape[0] + 1) // 2
    # the host builder's tree: same leaves, same topology, same leaf representatives at the same ordinals
    assert nl == ht.num_leaves, (nl, ht.num_leaves)
    hn = ht.nodes
    assert np.array_equal(nodes["right"], hn["right"])
    leaf = nodes["right"] == 0
    same_mean = np.all(nodes["mean"][leaf].view(np.uint64) == hn["mean"][leaf].view(np.uint64), axis=1)
    if name == "expline36":
        assert ctx.tree_build_stats()["max_level"] > 20
    # (equally spaced collinear points — three-point leaves whose outer members tie EXACTLY — included: with the centroid of a
    # small node added up in member order the tie breaks as on the host)
    assert same_mean.mean() >= 0.999, (same_mean.mean(), int((~same_mean).sum()))
    # ... and the same member order: the construction left the points where the host builder's in-place splits leave them
    # (utils.h:37-52), row for row — except that the host, like the reference, also writes a leaf's representative over the
    # leaf's first member (mad_tree.cpp:76-84)
    d_order = ctx.tree_build_points(pts.shape[0])
    h_order, _ = capi.host_tree_points(pts, B_MAX, B_MIN, 2)
    same_row = np.all(d_order.view(np.uint64) == h_order.view(np.uint64), axis=1)
    reps = keyset(hn["mean"][leaf])
    assert all(bytes(h_order[i].view(np.uint8)) in reps for i in np.flatnonzero(~same_row))
    assert keyset(d_order) == keyset(pts) and d_order.shape == pts.shape
    # bit-reproducible: a second build of the same cloud gives the same bytes
    t2, _ = ctx.tree_build(cid, B_MAX, B_MIN)
    assert ctx.tree_download(t2, nodes.shape[0]).tobytes() == nodes.tobytes()
    st = ctx.tree_build_stats()
    assert st["max_level"] < 96
    for t in (tid, t2):
        ctx.tree_release(t)
    ctx.cloud_release(cid)


def test_device_tree_matches_host_builder_on_many_full_size_scans(ctx, capsys):
    """Twelve full-size scans (two scenes, poses along the drive, one of them the keyframe map's first scan): on every one
    the device-built tree has the host builder's leaf count and `right` links, and at least 99.9 % of its leaf
    representatives at the same leaf ordinals (measured: all of them) — the member order of the reference's split
    (utils.h:37-52) is what "first member wins" (mad_tree.cpp:76-86) depends on."""
    scans = [synth.render_scan(synth.Scene(sc), synth.path_pose(2.5 * i), 700 + 13 * sc + i) for sc in (0, 3) for i in range(6)]
    worst, total_leaves, total_diff, bitwise_internal = 1.0, 0, 0, []
    d_bbox = d_nrm = 0.0
    n_loose = 0
    for pts in scans:
        ht, cid, tid, nodes = build_both(ctx, pts)
        hn = ht.nodes
        assert nodes.shape[0] == hn.shape[0] and np.array_equal(nodes["right"], hn["right"])
        leaf = nodes["right"] == 0
        same = np.all(nodes["mean"][leaf].view(np.uint64) == hn["mean"][leaf].view(np.uint64), axis=1)
        worst = min(worst, same.mean())
        total_leaves += int(leaf.sum())
        total_diff += int((~same).sum())
        bitwise_internal.append(np.all(nodes["mean"][~leaf].view(np.uint64) == hn["mean"][~leaf].view(np.uint64), axis=1).mean())
        assert same.mean() >= 0.999, (same.mean(), int((~same).sum()))
        # bbox0 (the planarity weight's input, mad_icp.cpp:97) and the normals agree as far as the eigen-decomposition's
        # conditioning lets last-bit differences of the covariance through (close eigenvalues: a direction moves by
        # eps x norm / gap)
        d_bbox = max(d_bbox, float(np.abs(nodes["bbox0"][leaf] - hn["bbox0"][leaf]).max()))
        dn = np.abs(nodes["dir"][leaf] - hn["dir"][leaf]).max(axis=1)
        d_nrm = max(d_nrm, float(dn.max()))
        n_loose += int((dn > 1e-9).sum())
        ctx.tree_release(tid)
        ctx.cloud_release(cid)
    with capsys.disabled():
        print("\n[device vs host builder, %d scans] leaf representatives that differ: %d of %d (worst scan %.5f equal); internal "
              "centroids bitwise equal: %.2f; largest difference of a leaf's bbox0 %.1e m, of a normal's component %.1e "
              "(%d leaves beyond 1e-9)"
              % (len(scans), total_diff, total_leaves, worst, float(np.mean(bitwise_internal)), d_bbox, d_nrm, n_loose))
    # (serial sums for the nodes of at most 32 points, round 4: their covariance is the host builder's bit for bit, so
    # even the leaves whose members are nearly collinear — smallest eigenvector left to rounding — agree)
    assert d_bbox <= 1e-9 and d_nrm <= 1e-8 and n_loose == 0
    assert float(np.mean(bitwise_internal)) >= 0.6   # (measured 0.77: the nodes of more than 32 points add in another shape)


@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65, 127, 129, 511, 512, 513, 514, 767, 769, 1023, 1025, 2047, 2048, 2049, 4095,
                               4097, 6143, 6145, 20001])
def test_device_tree_build_at_regime_boundaries(mctx, n):
    """Cloud sizes on both sides of every regime boundary of the device builder — four lanes / one wavefront (32 | 33), one
    wavefront / a team of four (512 | 513), one chunk / two (2048 | 2049), the lane-strided batches in between — on an
    anisotropic Gaussian cloud: exact properties, the host builder's topology and leaf representatives, and the
    construction's member order equal to the host builder's row for row (utils.h:37-52)."""
    ctx = mctx  # (the measurement build's context: madicp_debug_tree_build_points below)
    rng = np.random.default_rng(1000 + n)
    pts = rng.normal(size=(n, 3)) * [6.0, 2.5, 0.4] + [3.0, -2.0, 1.0]
    ht, cid, tid, nodes = build_both(ctx, pts, 0.2, 0.1)
    check_exact_properties(ctx, pts, tid, nodes)
    hn = ht.nodes
    assert nodes.shape[0] == hn.shape[0] and np.array_equal(nodes["right"], hn["right"])
    leaf = nodes["right"] == 0
    same = np.all(nodes["mean"][leaf].view(np.uint64) == hn["mean"][leaf].view(np.uint64), axis=1)
    assert same.mean() >= 0.995, (same.mean(), int((~same).sum()))
    d_order = ctx.tree_build_points(n)
    h_order, _ = capi.host_tree_points(pts, 0.2, 0.1, 2)
    same_row = np.all(d_order.view(np.uint64) == h_order.view(np.uint64), axis=1)
    reps = keyset(hn["mean"][leaf])
    assert all(bytes(h_order[i].view(np.uint8)) in reps for i in np.flatnonzero(~same_row))
    assert keyset(d_order) == keyset(pts)
    ctx.tree_release(tid)
    ctx.cloud_release(cid)


def test_device_tree_build_on_random_small_clouds(ctx):
    """Sixty random small clouds (blobs, sheets, lines, duplicates at random scales and thresholds, 1 .. 400 points) through
    the device builder: always a valid tree with the exact properties (preorder, leaf ordinals, every leaf mean a member of the
    cloud and its own nearest neighbour), the leaf count the host builder's to within one leaf in fifty, and the same bytes
    from the look-ahead entry."""
    r2 = np.random.default_rng(77)
    for i in range(60):
        n = int(r2.integers(1, 400))
        kind = int(r2.integers(4))
        c = r2.normal(size=(n, 3)) * r2.choice([0.01, 0.3, 5.0], size=3)
        if kind == 1:
            c[:, 2] = 0.0
        elif kind == 2:
            c[:, 1:] = 0.0
        elif kind == 3:
            c = np.repeat(c[: max(1, n // 4)], 4, axis=0)
        c = c + r2.normal(size=3) * 10.0
        b_max, b_min = float(r2.choice([1e-5, 0.05, 0.2, 1.0])), float(r2.choice([0.01, 0.1, 0.5]))
        r2.integers(3)  # (the host tests' parallel level: keeps the three tests on the same clouds)
        ht, cid, tid, nodes = build_both(ctx, c, b_max, b_min)
        check_exact_properties(ctx, c, tid, nodes)
        nl = (nodes.shape[0] + 1) // 2
        assert abs(nl - ht.num_leaves) <= max(2, ht.num_leaves // 50), (i, nl, ht.num_leaves)
        ctx.tree_build_begin(c, b_max, b_min)
        t2, nl2 = ctx.tree_build_end()
        assert nl2 == nl and ctx.tree_download(t2, nodes.shape[0]).tobytes() == nodes.tobytes(), i
        ctx.tree_release(t2)
        ctx.tree_release(tid)
        ctx.cloud_release(cid)


def test_dense_tree_self_query_is_exact(ctx):
    """apps/utils/tools/nn_search.py:55-61 on a device-built tree: b_max = 1e-5, every point queried, total error 0."""
    pts = street_problem(2)["query_scans"][0]
    cid = ctx.cloud_upload(pts)
    tid, nl = ctx.tree_build(cid, 1e-5, B_MIN)
    r = ctx.nn_search(tid, pts, want=("dist",))
    assert r["dist"].sum() == 0.0
    ctx.tree_release(tid)
    ctx.cloud_release(cid)


def test_registration_against_device_built_map(ctx):
    pb = synth.make_problem(4, seed=1, n_queries=1)
    dev_t, host_t = [], []
    for s, T in zip(pb["keyframe_scans"], pb["keyframe_poses"]):
        c = ctx.cloud_upload(s)
        t, _ = ctx.tree_build(c, B_MAX, B_MIN)
        ctx.tree_transform(t, T[:3, :3], T[:3, 3])
        ctx.cloud_release(c)
        dev_t.append(t)
        h = capi.HostTree(s, B_MAX, B_MIN, 2)
        h.transform(T[:3, :3], T[:3, 3])
        host_t.append(ctx.upload(h))
    scan = pb["query_scans"][0]
    qh = capi.HostTree(scan, B_MAX, B_MIN, 2)
    c = ctx.cloud_upload(scan)
    qt, nl = ctx.tree_build(c, B_MAX, B_MIN)
    T0, gt = pb["query_guess"][0], pb["query_gt"][0]
    rd = ctx.stream_collect(ctx.stream_submit_tree(qt, dev_t, T0, PARAMS, 15), nl)
    rh = ctx.stream_collect(ctx.stream_submit(qh.leaf_means(), host_t, T0, PARAMS, 15), qh.num_leaves)
    d = np.linalg.inv(rh["T"]) @ rd["T"]
    assert np.linalg.norm(d[:3, 3]) <= 1e-9   # (identical representatives, normals and extents to ~1e-11)
    assert np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1)) <= 1e-6
    for r in (rd, rh):
        assert np.linalg.norm((np.linalg.inv(gt) @ r["T"])[:3, 3]) <= 0.02
    assert abs(rd["n_matched"] / nl - rh["n_matched"] / qh.num_leaves) <= 0.01
    # the device-made top layout is the host-made one: same trees through the upload path, same bits out
    re_t = []
    for t in dev_t:
        nn, l_ = ctx.tree_info(t)
        re_t.append(ctx.tree_upload(ctx.tree_download(t, nn), l_))
    rr = ctx.stream_collect(ctx.stream_submit_tree(qt, re_t, T0, PARAMS, 15), nl)
    assert np.array_equal(rr["X"], rd["X"]) and np.array_equal(rr["H"], rd["H"]) and np.array_equal(rr["matched"], rd["matched"])
    for t in dev_t + host_t + re_t + [qt]:
        ctx.tree_release(t)
    ctx.cloud_release(c)


def test_top_layout_with_a_deep_small_sub_tree_born_during_the_chip_levels(ctx):
    """The LDS-staged top of a device-built tree is laid out INSIDE level launches of the construction (tb_level's first
    workgroup, three parts), which is only right if every node a part reads has been finished — and a node of level L is
    finished by step L + 5, not L: a small node born while the chip regime runs waits for step 6 and its descendants follow
    one step per level.  Here such a node exists: 400 points on a 60 m line, 300 m from a 60 k-point slab, split off at
    level 3 and ten levels deep — its level-11 nodes are made at step 14.  Checked: the host builder's topology, and the
    device-made top layout gives the bits of the host-made one (the same tree through the upload path) in a registration
    whose leaves walk both parts of the tree.  (A layout made too early is a RACE, not a certain failure: this input passes
    with the parts one step behind their levels more often than not; what caught that schedule was the 200-frame drive of
    test_device_front_end_over_a_long_drive, 1.8e-2 m off the host path.)"""
    rng = np.random.default_rng(11)
    slab = rng.uniform([-20, -20, -2], [20, 20, 2], size=(60000, 3))
    line = np.stack([np.linspace(300.0, 360.0, 400), 0.01 * rng.normal(size=400), 0.01 * rng.normal(size=400)], 1)
    pts = np.concatenate([slab, line])[rng.permutation(60400)]
    ht = capi.HostTree(pts, B_MAX, B_MIN, 2)
    cid = ctx.cloud_upload(pts)
    tid, nl = ctx.tree_build(cid, B_MAX, B_MIN)
    ctx.cloud_release(cid)
    assert nl == ht.num_leaves
    nodes = ctx.tree_download(tid, 2 * nl - 1)
    assert np.array_equal(nodes["right"], ht.nodes["right"])
    st = ctx.tree_build_stats()
    assert st["max_level"] >= 12  # (the line's sub-tree really is deep)
    re_t = ctx.tree_upload(nodes, nl)
    # moving set: the tree's own leaves, nudged — every leaf of the line and of the slab walks the staged top
    leaves = nodes["mean"][nodes["right"] == 0] + 0.01
    T0 = np.eye(4)
    T0[:3, 3] = [0.02, -0.01, 0.0]
    a = ctx.stream_collect(ctx.stream_submit(leaves, [tid], T0, PARAMS, 4), leaves.shape[0])
    b = ctx.stream_collect(ctx.stream_submit(leaves, [re_t], T0, PARAMS, 4), leaves.shape[0])
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["H"], b["H"]) and np.array_equal(a["matched"], b["matched"])
    assert a["n_matched"] > 0.5 * leaves.shape[0]
    ctx.tree_release(tid)
    ctx.tree_release(re_t)


def _pose(tx, ty, yaw, pitch):
    T = np.eye(4)
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    T[:3, 3] = [tx, ty, 0.01]
    return T


@pytest.mark.parametrize("motion", [(0.9, 0.05, 0.02, 0.03), (0.0, 0.0, 0.0, 0.0), (-1.4, 0.3, -0.2, 0.01)])
def test_deskew_matches_oracle(ctx, motion):
    scan = synth.make_problem(1, seed=2, n_queries=1)["query_scans"][0]
    Tp, Tn = np.eye(4), _pose(*motion)
    ref, vel = O.deskew(scan, Tp, Tn, 10.0)
    cid = ctx.cloud_upload(scan)
    chunks = ctx.cloud_deskew(cid, vel, 10.0, want_chunks=True)
    out = ctx.cloud_download(cid)
    assert out.shape == ref.shape
    assert keyset(out) == keyset(ref)          # every compensated point, bit for bit; order may differ among azimuth ties
    assert sorted(map(bytes, out.view(np.uint8).reshape(-1, 24))) == sorted(map(bytes, ref.view(np.uint8).reshape(-1, 24)))
    # time chunks in walk order (largest azimuth first): start at 0, move on by at most one per point (pipeline.cpp:109-118)
    assert chunks[0] in (0, 1) and chunks.max() <= 1024 and (np.diff(chunks) >= 0).all() and (np.diff(chunks) <= 1).all()
    ctx.cloud_release(cid)


@pytest.mark.parametrize("kitti", [0, 1])
def test_ingest_is_bit_identical(ctx, kitti):
    scan = street_problem(2)["query_scans"][0]
    rec = np.zeros((scan.shape[0] + 6, 4), np.float32)
    rec[:-6, :3] = scan.astype(np.float32)
    rec[:-6, 3] = 0.5
    rec[-6] = [np.nan, 1, 1, 0]
    rec[-5] = [1, 1, np.nan, 0]
    rec[-4] = [0.1, 0.1, 0.1, 0]      # below min_range
    rec[-3] = [500, 0, 0, 0]          # beyond max_range
    rec[-2] = [0, 0, 5, 0]            # on the z axis: the correction's rotation axis has zero length
    rec[-1] = [3, 4, 0, 0]
    ref = O.ingest_f32(rec, 0.7, 120.0, kitti)
    cid, kept = ctx.cloud_ingest_f32(rec, 0.7, 120.0, kitti)
    out = ctx.cloud_download(cid)
    assert kept == ref.shape[0] == out.shape[0]
    assert ((out == ref) | (np.isnan(out) & np.isnan(ref))).all()
    ctx.cloud_release(cid)


def test_ingest_accepts_wide_records(ctx):
    """records wider than a scratch point (x, y, z + 6 more floats = 36 bytes): first call on a fresh scratch layout"""
    rng = np.random.default_rng(9)
    rec = rng.normal(0, 8, (5000, 9)).astype(np.float32)
    ref = O.ingest_f32(rec, 0.7, 120.0, 0)
    c2 = ctx.__class__()
    try:
        cid, kept = c2.cloud_ingest_f32(rec, 0.7, 120.0, 0)
        out = c2.cloud_download(cid)
        assert kept == ref.shape[0] and (out == ref).all()
    finally:
        c2.close()


def test_two_contexts_on_two_threads(ctx):
    """the front-end state (resident clouds, builder scratch) belongs to its context: two contexts driven from two host
    threads build their own clouds' trees concurrently and get what a lone context gets"""
    import threading
    rng = np.random.default_rng(21)
    clouds = [rng.normal(0, 5, (30000, 3)) * [1, 1, 0.2], rng.normal(0, 9, (45000, 3)) * [1, 0.3, 1]]
    want = []
    for c in clouds:
        cid = ctx.cloud_upload(c)
        t, nl = ctx.tree_build(cid, B_MAX, B_MIN)
        want.append(nl)
        ctx.tree_release(t)
        ctx.cloud_release(cid)
    got, errs = [[], []], []

    def work(i):
        try:
            c2 = ctx.__class__()
            for _ in range(6):
                cid = c2.cloud_upload(clouds[i])
                t, nl = c2.tree_build(cid, B_MAX, B_MIN)
                got[i].append(nl)
                c2.tree_release(t)
                c2.cloud_release(cid)
            c2.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert got[0] == [want[0]] * 6 and got[1] == [want[1]] * 6


# ---- the device front-end behind Pipeline.compute (opt-in) -------------------------------------------------------------
N_FRAMES = 12


@pytest.fixture(scope="module")
def drive():
    scene = synth.Scene(0)
    return [synth.render_scan(scene, synth.path_pose(1.0 * i), 100 + i) for i in range(N_FRAMES)]


def _pose_err(Ta, Tb):
    d = np.linalg.inv(Ta) @ Tb
    return np.linalg.norm(d[:3, 3]), np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1))


def _jittered(scans, seed=0):
    """the same scans with 1e-7 m of noise: no two points share an azimuth any more, so std::sort's unspecified order among
    ties (which the synthetic scans' 64-point azimuth columns are full of) stops separating host and device deskew"""
    rng = np.random.default_rng(seed)
    return [sc + rng.normal(scale=1e-7, size=sc.shape) for sc in scans]


@pytest.mark.parametrize("deskew,jitter", [(False, False)])
def test_pipeline_with_device_front_end(natives, drive, deskew, jitter, capsys):
    """Pipeline.compute with tree construction (and deskew) on the device against the same Pipeline on the host path.
    The host path is the one held to 1e-5 against the oracle (tests/test_gpu_pipeline_fullsize.py).  Device-built trees
    have the host builder's member order and leaf representatives, and the nodes of at most 32 points — nearly all leaves —
    the host builder's centroid and covariance bit for bit (serial sums in member order); what differs is last bits of the
    larger nodes.  The two trajectories agree to 1e-9 m / 1e-6 rad at every frame (measured 8e-14 m over this drive; 4.5e-6
    before the serial sums, 6e-4 before the member order), with the same keyframe decisions and inlier ratios within 1 %.  (Round 5:
    deskew = true is no longer held to a bar BETWEEN the product's two paths — the reference does not reproduce itself there
    beyond millimetres — but each path against the oracle, inside the oracle's own measured envelope:
    tests/test_gpu_frontend_oracle.py, tests/envelope.py.)"""
    import time

    from mad_icp.src.pybind import pypeline as m

    args = (10.0, deskew, B_MAX, 0.1, 0.8, B_MIN, 0.02, 16, 8, False)
    host, dev = m.Pipeline(*args), m.Pipeline(*args)
    assert dev.deviceFrontEnd()  # the default (round 5: for deskew = false; round 6: everywhere)
    host.setDeviceFrontEnd(False)
    dev.setDeviceFrontEnd(True)
    assert dev.deviceFrontEnd() and not host.deviceFrontEnd()
    worst = (0.0, 0.0)
    t_dev, t_host = [], []
    scans = _jittered(drive) if jitter else drive
    bar_t, bar_a = (1e-9, 1e-6) if not deskew else (1e-2, 1e-3)
    for i, s in enumerate(scans):
        t = time.perf_counter()
        host.compute(0.1 * i, s)
        t_host.append(time.perf_counter() - t)
        t = time.perf_counter()
        dev.compute(0.1 * i, s)
        t_dev.append(time.perf_counter() - t)
        dt, da = _pose_err(np.asarray(host.currentPose()), np.asarray(dev.currentPose()))
        worst = (max(worst[0], dt), max(worst[1], da))
        assert dt <= bar_t and da <= bar_a, (i, dt, da)
        assert host.currentID() == dev.currentID() and host.keyframeID() == dev.keyframeID()
        if i > 0:
            assert abs(host.lastInliersRatio() - dev.lastInliersRatio()) <= 0.01
    # the leaves can still be read back (downloaded on demand)
    cl = np.asarray(dev.currentLeaves())
    assert cl.ndim == 2 and cl.shape[1] == 3 and abs(cl.shape[0] - np.asarray(host.currentLeaves()).shape[0]) <= cl.shape[0] // 100
    ml = np.asarray(dev.modelLeaves())
    assert ml.shape[0] >= cl.shape[0] // 2
    gt = np.linalg.inv(synth.path_pose(0.0)) @ synth.path_pose(1.0 * (N_FRAMES - 1))
    if not deskew:  # (the synthetic scans are instantaneous: compensating them for motion moves them)
        assert np.linalg.norm(np.asarray(dev.currentPose())[:3, 3] - gt[:3, 3]) < 0.1
    with capsys.disabled():
        print("\n[pipeline, device front-end, deskew=%s%s] worst deviation from the host path %.2e m / %.2e rad; per frame: device "
              "front-end %.2f ms (tree+deskew %.2f ms), host path %.2f ms (build %.2f ms)"
              % (deskew, " (jittered: no azimuth ties)" if jitter else "", worst[0], worst[1], 1e3 * np.median(t_dev[2:]), dev.lastBuildMs(), 1e3 * np.median(t_host[2:]),
                 host.lastBuildMs()))


@pytest.mark.parametrize("deskew,jitter,n_frames", [(False, False, 200)])
def test_device_front_end_over_a_long_drive(natives, deskew, jitter, n_frames, capsys):
    """The acceptance bar of the device front-end over a long full-size drive (1 m
    per frame, 120 k-point scans), device front-end next to the host path — the one held to 1e-5 against the oracle:
      * the two trajectories within 1e-9 m of each other at EVERY frame (measured 8e-13 m at most over the 200 frames:
        far inside the 1e-5 m of the north-star tolerance) — device-built trees have the host builder's member order and
        leaf representatives, and its centroids and covariances bit for bit for the nodes of at most 32 points;
      * final and RMS translation error against ground truth equal to the host path's to 1 mm;
      * the same keyframes promoted at the same frames.
    (Round 5: the deskewed 100-frame drives moved to tests/test_gpu_frontend_oracle.py, where each path is held inside the
    envelope the oracle pipeline shows against ITSELF under a thread-count or 1-ulp change, instead of to 5 cm of the other.)"""
    from mad_icp.src.pybind import pypeline as m

    scene = synth.Scene(0)
    args = (10.0, deskew, B_MAX, 0.1, 0.8, B_MIN, 0.02, 16, 16, False)
    host, dev = m.Pipeline(*args), m.Pipeline(*args)
    host.setDeviceFrontEnd(False)
    dev.setDeviceFrontEnd(True)
    T0inv = np.linalg.inv(synth.path_pose(0.0))
    eh, ed, between, kf_h, kf_d = [], [], [], [], []
    rng = np.random.default_rng(3)
    for i in range(n_frames):
        sc = full_scan(0, 1.0 * i, 100 + i)
        if jitter:
            sc = sc + rng.normal(scale=1e-7, size=sc.shape)
        host.compute(0.1 * i, sc)
        dev.compute(0.1 * i, sc)
        gt = T0inv @ synth.path_pose(1.0 * i)
        Th, Td = np.asarray(host.currentPose()), np.asarray(dev.currentPose())
        eh.append(np.linalg.norm((np.linalg.inv(gt) @ Th)[:3, 3]))
        ed.append(np.linalg.norm((np.linalg.inv(gt) @ Td)[:3, 3]))
        between.append(np.linalg.norm((np.linalg.inv(Th) @ Td)[:3, 3]))
        kf_h.append(host.keyframeID())
        kf_d.append(dev.keyframeID())
    eh, ed, between = np.array(eh), np.array(ed), np.array(between)
    rms_h, rms_d = np.sqrt((eh ** 2).mean()), np.sqrt((ed ** 2).mean())
    with capsys.disabled():
        print("\n[front-end acceptance, %d frames, deskew=%s%s] error vs ground truth: host final %.4f rms %.4f m | device final %.4f "
              "rms %.4f m | device vs host max %.3e m (median %.3e) | keyframe id differs on %d frames (%d / %d promoted)"
              % (n_frames, deskew, " jittered" if jitter else "", eh[-1], rms_h, ed[-1], rms_d, between.max(), np.median(between),
                 int(np.sum(np.array(kf_h) != np.array(kf_d))), len(set(kf_h)), len(set(kf_d))))
    if not deskew:
        assert between.max() <= 1e-9
        assert abs(ed[-1] - eh[-1]) <= 1e-3 and abs(rms_d - rms_h) <= 1e-3
        assert kf_h == kf_d
    else:
        assert ed[-1] <= 1.02 * eh[-1] + 1e-3 and rms_d <= 1.02 * rms_h + 1e-3
        assert between.max() <= 5e-2
        assert len(set(kf_h)) == len(set(kf_d))
        assert np.sum(np.array(kf_h) != np.array(kf_d)) <= max(1, n_frames // 100)


def test_pipeline_compute_records(natives, drive):
    """computeRecords (float32 sensor records in, everything on the device) == compute() on the records filtered and
    converted on the host, both with the device front-end: identical trajectories."""
    from mad_icp.src.pybind import pypeline as m

    args = (10.0, False, B_MAX, 0.1, 0.8, B_MIN, 0.02, 8, 4, False)
    a, b = m.Pipeline(*args), m.Pipeline(*args)
    b.setDeviceFrontEnd(True)
    for i, s in enumerate(drive[:5]):
        rec = np.zeros((s.shape[0], 4), np.float32)
        rec[:, :3] = s.astype(np.float32)
        a.computeRecords(0.1 * i, rec, 0.7, 120.0, False)
        b.compute(0.1 * i, O.ingest_f32(rec, 0.7, 120.0, False))
        assert np.array_equal(np.asarray(a.currentPose()), np.asarray(b.currentPose()))


def test_front_end_abi_errors_are_loud(ctx):
    """Bad arguments to the additive entry points raise with the library's message; nothing is left half-made."""
    with pytest.raises(capi.MadIcpError, match="unknown cloud id"):
        ctx.tree_build(987654, B_MAX, B_MIN)
    with pytest.raises(capi.MadIcpError, match="unknown cloud id"):
        ctx.cloud_release(987654)
    with pytest.raises(capi.MadIcpError, match="unknown cloud id"):
        ctx.cloud_deskew(987654, np.zeros(6), 10.0)
    cid = ctx.cloud_upload(np.array([[1.0, 2.0, 3.0], [2.0, 3.0, 4.0]]))
    with pytest.raises(capi.MadIcpError, match="sensor_hz"):
        ctx.cloud_deskew(cid, np.zeros(6), 0.0)
    out = np.empty((5, 3))
    rc = capi.hip_lib().madicp_cloud_download(ctx._h, cid, out.ctypes.data_as(capi._dp), 5)
    assert rc != 0 and b"mismatch" in capi.hip_lib().madicp_last_error()
    ctx.cloud_release(cid)
    with pytest.raises(capi.MadIcpError, match="no point survives"):
        ctx.cloud_ingest_f32(np.full((10, 4), 500.0, np.float32), 0.7, 120.0, 0)
    with pytest.raises(ValueError):
        ctx.cloud_ingest_f32(np.zeros((10, 2), np.float32), 0.7, 120.0, 0)
    with pytest.raises(capi.MadIcpError, match="unknown tree id"):
        ctx.tree_info(987654)
    # and the context still works afterwards
    c2 = ctx.cloud_upload(street_problem(2)["query_scans"][0])
    t2, nl = ctx.tree_build(c2, B_MAX, B_MIN)
    assert nl > 100
    ctx.tree_release(t2)
    ctx.cloud_release(c2)


def test_deskew_is_bit_identical_without_azimuth_ties(ctx):
    """With distinct azimuths (a random cloud: no two points share atan2(y, x)) there is nothing std::sort's instability
    could reorder, and the device deskew is the oracle's row for row, bit for bit — the device atan2 only has to ORDER
    the points and place them against the chunk thresholds like libm's does."""
    rng = np.random.default_rng(21)
    pts = rng.normal(size=(60000, 3)) * [30.0, 30.0, 2.0]
    az = np.arctan2(pts[:, 1], pts[:, 0])
    assert np.unique(az).size == az.size
    ref, vel = O.deskew(pts, np.eye(4), _pose(0.8, -0.1, 0.03, 0.01), 10.0)
    cid = ctx.cloud_upload(pts)
    ctx.cloud_deskew(cid, vel, 10.0)
    out = ctx.cloud_download(cid)
    assert np.array_equal(out, ref)
    ctx.cloud_release(cid)


# ---- the look-ahead form of the device build (madicp_tree_build_begin / _end) -----------------------------------------------
def test_look_ahead_build_is_the_synchronous_build(ctx):
    """madicp_tree_build_begin .. _end give the tree of madicp_cloud_upload + madicp_tree_build bit for bit — with
    registrations, uploads, transforms and searches of OTHER trees running on the context between the two calls (the
    construction is on a stream of its own).  The builder's scratch has one owner: a second _begin, a synchronous build, an
    ingest or a deskew in between are refused with the library's message, and a cancelled look-ahead leaves no trace."""
    pb = street_problem(2)
    scan = pb["query_scans"][0]
    other = pb["keyframe_scans"][0]
    cid = ctx.cloud_upload(scan)
    t_sync, nl_sync = ctx.tree_build(cid, B_MAX, B_MIN)
    ref = ctx.tree_download(t_sync, 2 * nl_sync - 1)
    # a resident map to keep the device busy in between
    kf = capi.HostTree(other, B_MAX, B_MIN, 2)
    Tk = pb["keyframe_poses"][0]
    tk = ctx.upload(kf)
    ctx.tree_transform(tk, Tk[:3, :3], Tk[:3, 3])
    moving = capi.HostTree(scan, B_MAX, B_MIN, 2).leaf_means()
    tick = ctx.stream_submit(moving, [tk], pb["query_guess"][0], PARAMS, 15)
    base = ctx.stream_collect(tick, moving.shape[0])

    for rep in range(3):
        ctx.tree_build_begin(scan, B_MAX, B_MIN)
        with pytest.raises(capi.MadIcpError, match="look-ahead tree build is in flight"):
            ctx.tree_build_begin(scan, B_MAX, B_MIN)
        with pytest.raises(capi.MadIcpError, match="look-ahead tree build is in flight"):
            ctx.tree_build(cid, B_MAX, B_MIN)
        with pytest.raises(capi.MadIcpError, match="look-ahead tree build is in flight"):
            ctx.cloud_deskew(cid, np.zeros(6), 10.0)
        with pytest.raises(capi.MadIcpError, match="look-ahead tree build is in flight"):
            ctx.cloud_ingest_f32(np.ones((10, 4), np.float32), 0.7, 120.0, 0)
        # everything else goes on
        tick = ctx.stream_submit(moving, [tk], pb["query_guess"][0], PARAMS, 15)
        ctx.nn_search(tk, scan[:1000], want=("leaf",))
        r = ctx.stream_collect(tick, moving.shape[0])
        assert np.array_equal(r["X"], base["X"]) and np.array_equal(r["H"], base["H"])
        c3 = ctx.cloud_upload(other)
        ctx.cloud_release(c3)
        if rep == 1:
            ctx.tree_build_cancel()
            ctx.tree_build_cancel()  # (no-op without one)
            with pytest.raises(capi.MadIcpError, match="no look-ahead tree build in flight"):
                ctx.tree_build_end()
            continue
        t_la, nl_la = ctx.tree_build_end()
        assert nl_la == nl_sync
        got = ctx.tree_download(t_la, 2 * nl_la - 1)
        assert got.tobytes() == ref.tobytes()
        # and it is a tree like any other: searched, registered against, released
        l2 = ctx.nn_search(t_la, scan[:1000], want=("leaf",))["leaf"]
        l1 = ctx.nn_search(t_sync, scan[:1000], want=("leaf",))["leaf"]
        assert np.array_equal(l1, l2)
        ctx.tree_release(t_la)
    # the synchronous entry works again
    t4, nl4 = ctx.tree_build(cid, B_MAX, B_MIN)
    assert ctx.tree_download(t4, 2 * nl4 - 1).tobytes() == ref.tobytes()
    for t in (t4, t_sync, tk):
        ctx.tree_release(t)
    ctx.cloud_release(cid)


def test_pipeline_device_front_end_look_ahead(natives, drive, capsys):
    """Pipeline with the device front-end on, prefetch(i + 1) issued before compute(i): the construction of the next scan's
    tree runs on the build stream beside the registration of this one.  Device builds are bit-reproducible, so the
    trajectory is the one of the same Pipeline without look-ahead, bit for bit; a second Pipeline of the process that builds
    synchronously in between takes the scratch (the first one's ticket goes stale and it builds when its scan comes) and
    both still produce their own trajectories."""
    import time

    from mad_icp.src.pybind import pypeline as m

    args = (10.0, False, B_MAX, 0.1, 0.8, B_MIN, 0.02, 16, 8, False)
    plain, ahead = m.Pipeline(*args), m.Pipeline(*args)
    for p in (plain, ahead):
        p.setDeviceFrontEnd(True)
    t_plain, t_ahead = [], []
    for i, s in enumerate(drive):
        t = time.perf_counter()
        plain.compute(0.1 * i, s)
        t_plain.append(time.perf_counter() - t)
    ahead.prefetch(drive[0])
    for i, s in enumerate(drive):
        t = time.perf_counter()
        if i + 1 < len(drive):
            ahead.prefetch(drive[i + 1])
        ahead.compute(0.1 * i, s)
        t_ahead.append(time.perf_counter() - t)
    assert np.array_equal(np.asarray(ahead.trajectory()), np.asarray(plain.trajectory()))
    assert ahead.keyframeID() == plain.keyframeID()
    assert ahead.lookAheadHits() == len(drive) and plain.lookAheadHits() == 0
    # a caller whose FIRST scan comes without a prefetch is one ahead from there on: the construction in flight at a miss is
    # for the next scan and must be kept (dropping it left the pipeline permanently one behind: every frame a miss)
    late = m.Pipeline(*args)
    late.setDeviceFrontEnd(True)
    for i, s in enumerate(drive):
        if i + 1 < len(drive):
            late.prefetch(drive[i + 1])
        late.compute(0.1 * i, s)
    assert np.array_equal(np.asarray(late.trajectory()), np.asarray(plain.trajectory()))
    assert late.lookAheadHits() == len(drive) - 1
    # ... and on the host path (keyed look-aheads)
    hp, hl = m.Pipeline(*args), m.Pipeline(*args)
    hp.setDeviceFrontEnd(False)
    hl.setDeviceFrontEnd(False)
    for i, s in enumerate(drive[:8]):
        hp.compute(0.1 * i, s)
        if i + 2 < 8:
            hl.prefetch(drive[i + 2])
        hl.compute(0.1 * i, s)
    assert np.array_equal(np.asarray(hl.trajectory()), np.asarray(hp.trajectory()))
    assert hl.lookAheadHits() == 6
    # two Pipelines, one looking ahead, the other building synchronously in between
    a, b = m.Pipeline(*args), m.Pipeline(*args)
    a.setDeviceFrontEnd(True)
    b.setDeviceFrontEnd(True)
    a.prefetch(drive[0])
    for i, s in enumerate(drive[:6]):
        if i + 1 < 6:
            a.prefetch(drive[i + 1])
        b.compute(0.1 * i, s)  # cancels a's look-ahead
        a.compute(0.1 * i, s)
    ref = np.asarray(plain.trajectory())[:6]
    assert np.array_equal(np.asarray(a.trajectory()), ref) and np.array_equal(np.asarray(b.trajectory()), ref)
    with capsys.disabled():
        print("\n[pipeline, device front-end] mean per frame %.2f ms = %.0f frames/s; with prefetch(next) before compute: %.2f ms "
              "= %.0f frames/s" % (1e3 * np.mean(t_plain[3:]), 1.0 / np.mean(t_plain[3:]),
                                   1e3 * np.mean(t_ahead[3:-1]), 1.0 / np.mean(t_ahead[3:-1])))


def test_bindings_read_the_callers_points_only_during_the_call(natives, drive):
    """compute / prefetch are bound on a VIEW of the caller's points (Pipeline::computeView / prefetchView; the reference's
    by-value binding, pypeline.cpp:69, copies the container per call).  What the caller may rely on is what a by-value call
    gave: the memory is read during the call only — a scan handed to prefetch() and overwritten afterwards is still the scan the
    look-ahead was built from, whatever form it came in (VectorEigen3d, float64 array, float32 / strided array through
    forcecast) — and every form lands on the same trajectory, bit for bit."""
    from mad_icp.src.pybind import pypeline as m

    args = (10.0, False, B_MAX, 0.1, 0.8, B_MIN, 0.02, 16, 8, False)
    frames = drive[:8]
    ref = m.Pipeline(*args)
    for i, s in enumerate(frames):
        ref.compute(0.1 * i, m.VectorEigen3d(s))
    want = np.asarray(ref.trajectory())

    def run(wrap):
        pl = m.Pipeline(*args)
        pl.prefetch(wrap(frames[0]))
        for i, s in enumerate(frames):
            if i + 1 < len(frames):
                nxt = wrap(frames[i + 1])
                pl.prefetch(nxt)
                if isinstance(nxt, np.ndarray):
                    nxt[...] = 0.0  # the caller's buffer is the caller's again
                else:
                    nxt.clear()
            cur = wrap(s)
            pl.compute(0.1 * i, cur)
        assert pl.lookAheadHits() == len(frames)
        return np.asarray(pl.trajectory())

    assert np.array_equal(run(lambda s: s.copy()), want)  # float64 array, read in place
    assert np.array_equal(run(lambda s: m.VectorEigen3d(s)), want)  # the reference's container
    wide = lambda s: np.concatenate([s, np.ones((len(s), 1))], axis=1)[:, :3]  # noqa: E731  (a strided view: forcecast copies)
    assert np.array_equal(run(wide), want)
    # float32 input is converted by the binding (as pybind's forcecast always did): another cloud, so only self-consistency
    f32 = [s.astype(np.float32) for s in frames]
    a, b = m.Pipeline(*args), m.Pipeline(*args)
    for i, s in enumerate(f32):
        a.compute(0.1 * i, s)
        b.compute(0.1 * i, s.astype(np.float64))
    assert np.array_equal(np.asarray(a.trajectory()), np.asarray(b.trajectory()))
    with pytest.raises(Exception):
        m.Pipeline(*args).compute(0.0, m.VectorEigen3d())
    with pytest.raises(Exception):
        m.Pipeline(*args).compute(0.0, np.zeros((0, 3)))
    with pytest.raises(Exception):
        m.Pipeline(*args).compute(0.0, np.zeros((5, 4)))


def test_float_exact_clouds_cross_pcie_as_floats_and_arrive_as_the_same_doubles(ctx):
    """Option "upload_f32" (default on): a cloud whose coordinates are all exactly floats — what a sensor driver, a KITTI .bin or
    a PointCloud2 delivers once the caller has converted it to double — is staged and sent as floats and widened on the device.
    The resident cloud is the caller's doubles bit for bit (-0.0 and infinities included), a cloud with ONE value that is not a
    float (NaN, a genuine double, a value beyond the float range) goes the plain way — from that piece on —, and the tree
    built from either is the same array."""
    rng = np.random.default_rng(12)
    base = (rng.normal(size=(50_000, 3)) * [20.0, 15.0, 2.0]).astype(np.float32).astype(np.float64)
    base[7] = [-0.0, np.inf, -np.inf]
    cases = {"float-exact": base.copy()}
    c = base.copy(); c[40_001, 1] = np.nextafter(c[40_001, 1], 1.0); cases["a double in the second piece"] = c
    c = base.copy(); c[3, 0] = np.nan; cases["a NaN in the first piece"] = c
    c = base.copy(); c[10, 2] = 1e300; cases["beyond the float range"] = c
    c = base.copy(); c[9, 0] = 1e-320; cases["a double denormal"] = c
    cases["genuine doubles"] = rng.normal(size=(50_000, 3))
    cases["small (below the threshold of the float path)"] = base[:1000].copy()
    for name, pts in cases.items():
        for opt in (1, 0):
            ctx.set_option("upload_f32", opt)
            cid = ctx.cloud_upload(pts)
            back = ctx.cloud_download(cid)
            ctx.cloud_release(cid)
            assert np.array_equal(back.view(np.uint64), pts.view(np.uint64)), (name, opt)
    # the tree of a float-exact scan: the same array both ways (and the look-ahead entry stages the same way)
    from mad_icp_amd import synth

    scan = synth.render_scan(synth.Scene(2), synth.path_pose(3.0), 77).astype(np.float32).astype(np.float64)
    trees = []
    for opt in (1, 0):
        ctx.set_option("upload_f32", opt)
        cid = ctx.cloud_upload(scan)
        tid, nl = ctx.tree_build(cid, B_MAX, B_MIN)
        trees.append(ctx.tree_download(tid, 2 * nl - 1))
        ctx.tree_release(tid)
        ctx.cloud_release(cid)
    ctx.set_option("upload_f32", 1)
    ctx.tree_build_begin(scan, B_MAX, B_MIN)
    tid, nl = ctx.tree_build_end()
    trees.append(ctx.tree_download(tid, 2 * nl - 1))
    ctx.tree_release(tid)
    assert trees[0].tobytes() == trees[1].tobytes() == trees[2].tobytes()
