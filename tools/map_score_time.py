"""What scoring many pose hypotheses against the voxel map costs: the frame with every new option off against the parent commit's
frame, one Context.map_score_poses against K sequential scoring calls of Context.map_query, and one Pipeline.mapRelocalize.

  python tools/map_score_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/map_score_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)

The scans are the 120 k-point synthetic drive of tools/map_prune_time.py (22-byte XYZIRT records, 1 m per frame), fed to default
Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive, `repeats` drives each:

  (a) parent_off / child_off   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call, accumulation off — of
                    ANOTHER built tree of this project (--parent TREE: the parent commit's) and of THIS tree, each in a child
                    process per drive (this file with --frame-only, which touches nothing the parent lacks): child against child.
  (b) score_K{K}_s{stride}_r{reach}   one Context.map_score_poses of the last scan (resident) against the 0.2 m map of the whole
                    drive, the map built outside the clock, at K = 1, 8, 64, 512 hypotheses (mad_icp_amd.relocalize.pose_grid around
                    the scan's pose, the pose itself first), stride 1 and 8, reach 0 and 1: a host clock around the call, which
                    ends in its one host synchronisation.
      seq_K{K}_s{stride}_r{reach}     the same counts by K sequential Context.map_query(per_point=False) calls — the parent
                    commit's entry point, unchanged — on the same cloud subsampled on the host and uploaded outside the clock.
                    The two must give the same (K, 3) counts (asserted).
  (c) relocalize_K512_r4   one Pipeline.mapRelocalize(scan, 512 hypotheses, refine=4, iterations=10, stride=8, reach=1) of the last
                    scan against the moments map the Pipeline itself accumulated over the drive: the upload, the scoring call,
                    four registrations.

The first two frames of a drive are left out; per drive the mean over frames, then median / p10 / p90 over the drives.  Prints one
JSON line.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("MADICP_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mad_icp_amd import capi  # noqa: E402
from map_prune_time import B_MAX, B_MIN, B_RATIO, HI, LO, RHO_KER, VOXEL, K, make_drive, ms, stats  # noqa: E402

MAX_DIST = 0.1
POSE_COUNTS, STRIDES, REACHES = (1, 8, 64, 512), (1, 8), (0, 1)


def hypotheses(T, count):
    """the first `count` of a 1 m / 10 degree grid around T (T itself first)"""
    from mad_icp_amd.relocalize import pose_grid

    return np.ascontiguousarray(pose_grid(T, 5.0, 1.0, np.deg2rad(20.0), 2)[:count])


def score_legs(ctx, clouds):
    """(b): the last scan against the map of all of them"""
    pts, T = clouds[-1]
    out = {}
    cids = [ctx.cloud_upload(p) for p, _ in clouds]
    subs = {s: ctx.cloud_upload(np.ascontiguousarray(pts[::s])) for s in STRIDES}
    own = ctx.map_create(VOXEL, 1 << 18, 1 << 24)
    try:
        for cid, (_, Tk) in zip(cids, clouds):
            ctx.map_insert_cloud(own, cid, Tk[:3, :3], Tk[:3, 3])
        for count in POSE_COUNTS:
            G = hypotheses(T, count)
            assert G.shape[0] == count
            for stride in STRIDES:
                for reach in REACHES:
                    tag = "K%d_s%d_r%d" % (count, stride, reach)
                    ctx.map_score_poses(own, cids[-1], G, reach, MAX_DIST, stride)  # (warm: the pooled scratch exists)
                    t1 = time.perf_counter()
                    got = ctx.map_score_poses(own, cids[-1], G, reach, MAX_DIST, stride)
                    t2 = time.perf_counter()
                    ctx.map_query(own, subs[stride], G[0, :3, :3], G[0, :3, 3], reach, MAX_DIST, per_point=False)
                    t3 = time.perf_counter()
                    seq = [ctx.map_query(own, subs[stride], X[:3, :3], X[:3, 3], reach, MAX_DIST, per_point=False) for X in G]
                    t4 = time.perf_counter()
                    assert np.array_equal(got, np.array(seq, np.uint64)), "the batched counts differ from the sequential queries' (%s)" % tag
                    out["score_" + tag], out["seq_" + tag] = (t2 - t1) * 1e3, (t4 - t3) * 1e3
        own_pose = ctx.map_score_poses(own, cids[-1], hypotheses(T, 1), 1, MAX_DIST, 1)[0]
        out["shape"] = {"rows": ctx.map_size(own), "points": int(pts.shape[0]), "counts_pose0_s1_r1": [int(v) for v in own_pose]}
    finally:
        ctx.map_release(own)
        for cid in cids + list(subs.values()):
            ctx.cloud_release(cid)
    return out


def main():
    argv = sys.argv[1:]
    frame_only = "--frame-only" in argv
    parent = None
    if "--parent" in argv:
        at = argv.index("--parent")
        parent = os.path.abspath(argv[at + 1])
        del argv[at:at + 2]
    args = [a for a in argv if not a.startswith("--")]
    frames = int(args[0]) if len(args) > 0 else 16
    repeats = int(args[1]) if len(args) > 1 else 5
    from mad_icp.src.pybind import pypeline as pm

    drive = make_drive(frames)
    threads = min(os.cpu_count() or 1, 16)

    def pipeline():
        return pm.Pipeline(10.0, True, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, K, threads, False)

    def plain_drive(keep=None):
        pl = pipeline()
        if keep is not None:
            pl.setKeepScan(True)
        ts = []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
            if keep is not None:
                keep.append((pl.registeredScan(0.0, "sensor").astype(np.float64), np.asarray(pl.currentPose()).copy()))
        return ms(ts)

    if frame_only:  # (what --parent runs in the other tree: warm-up drives, then `repeats` timed ones)
        plain_drive()
        plain_drive()
        print(json.dumps({"off": [plain_drive() for _ in range(repeats)]}))
        return

    def child_drive(tree):
        env = dict(os.environ, MADICP_TREE=tree, PYTHONPATH=tree)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(frames), "1", "--frame-only"], env=env, cwd=tree,
                             capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])["off"][0]

    def relocalize_leg():
        """(c): the Pipeline's own moments map of the drive, its last scan, 512 hypotheses around its last pose"""
        pl = pipeline()
        pl.setKeepScan(True)
        pl.setMapAccumulation(VOXEL, moments=1 << 20)
        for i, rec in enumerate(drive):
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
        scan = pl.registeredScan(0.0, "sensor").astype(np.float64)
        G = hypotheses(np.asarray(pl.currentPose()), 512)
        kw = dict(refine=4, iterations=10, stride=8, reach=1, max_dist=MAX_DIST)
        pl.mapRelocalize(scan, G, **kw)
        t1 = time.perf_counter()
        got = pl.mapRelocalize(scan, G, **kw)
        t2 = time.perf_counter()
        return (t2 - t1) * 1e3, {"rows": int(pl.mapSize()), "points": int(scan.shape[0]), "index": got["index"].tolist(), "best": int(got["best"]),
                                 "within": got["scores"][:, 2].tolist(), "closing_inliers": got["counts"][:, 3].tolist()}

    ctx = capi.Context.borrowed()
    plain_drive()  # (the first drive of a process pays for the pool's and the builder's first allocations)
    if parent:
        child_drive(parent)
    res = {k: [] for k in ("parent_off", "child_off", "relocalize_K512_r4")}
    shape, reloc = {}, {}
    for r in range(repeats):
        print("map_score_time: drive set %d of %d" % (r + 1, repeats), file=sys.stderr, flush=True)
        if parent:
            res["parent_off"].append(child_drive(parent))
            res["child_off"].append(child_drive(ROOT))
        kept = []
        plain_drive(keep=kept)
        legs = score_legs(ctx, kept)
        shape = legs.pop("shape")
        for k, v in legs.items():
            res.setdefault(k, []).append(v)
        t, reloc = relocalize_leg()
        res["relocalize_K512_r4"].append(t)

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "voxel": VOXEL, "max_dist": MAX_DIST, "batched_counts_equal_sequential": True}
    for k, v in res.items():
        if v:
            out[k] = stats(v)
    out["score_shape"] = shape
    out["relocalize"] = reloc
    print(json.dumps(out))


if __name__ == "__main__":
    main()
