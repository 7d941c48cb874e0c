"""What pruning the voxel map costs: the frame with Pipeline.setMapRange off against the parent commit's frame, the frame with a range
that prunes during the drive, one Context.map_prune alone against today's only alternative (clear + re-fold), one process.

  python tools/map_prune_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/map_prune_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)

The scans are the 120 k-point synthetic drive of tools/map_accumulate_time.py (22-byte XYZIRT records, 1 m per frame), fed to default
Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive, `repeats` drives each:

  (i)   off / map   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call (it returns after the result has
                    been read back: a synchronised time) — of a Pipeline with accumulation off, and of one with
                    setMapAccumulation(0.2) and NO range.
        parent_*    --parent TREE: the same two frames of ANOTHER built tree of this project (the parent commit's), this file run
                    with --frame-only in a child process per drive, interleaved with the legs above — the same box, the same
                    session.  --frame-only touches nothing the parent lacks.
        child_*     ... and of THIS tree run the same way, in a child process per drive: the like-for-like partner of parent_*
                    (the legs of this process share it with every other leg's Pipelines, maps and allocations; a child has
                    made two warm-up drives and nothing else).
  (ii)  ranged      the frame of a Pipeline with setMapAccumulation(0.2) and setMapRange(RANGE): the drive advances 1 m per frame
                    and RANGE / 4 = 5 m, so the map is pruned on every fifth frame; the prunes and the rows removed are reported.
                    All legs must end on the same pose bit for bit (asserted).
  (iii) prune / clear_refold   one Context.map_prune alone on a map of the tool's own — the drive's final 0.2 m map (every frame's
                    compensated scan folded at its pose), centre the last pose, radius RANGE; and a synthetic map of 2^20 rows (a
                    1.5 m lattice folded in clouds of 2^17 points, about half of it kept) — against what a consumer can do today:
                    Context.map_clear + the re-fold of the last cloud.  Each repeat rebuilds the map first, outside the clock.

The first two frames of a drive (no deskew yet, first allocations) are left out; per drive the mean over frames, then median / p10 /
p90 over the drives.  Prints one JSON line.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("MADICP_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mad_icp_amd import capi, synth  # noqa: E402

B_MAX, B_MIN, RHO_KER, B_RATIO, K = 0.2, 0.1, 0.1, 0.02, 16
LO, HI = 0.7, 120.0
VOXEL, RANGE = 0.2, 20.0
XYZIRT = np.dtype(dict(names=["x", "y", "z", "intensity", "ring", "time"], formats=["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"],
                       offsets=[0, 4, 8, 12, 16, 18], itemsize=22))


def make_drive(frames):
    scene = synth.Scene(0)
    rng = np.random.default_rng(0)
    drive = []
    for i in range(frames):
        sc = synth.render_scan(scene, synth.path_pose(1.0 * i), 100 + i).astype(np.float32)
        n_bad = sc.shape[0] // 33
        bad = rng.normal(size=(n_bad, 3)).astype(np.float32)
        bad *= (np.where(rng.integers(2, size=n_bad) == 0, 0.2, 400.0) / np.linalg.norm(bad, axis=1))[:, None].astype(np.float32)
        xyz = np.insert(sc, rng.integers(0, sc.shape[0], size=n_bad), bad, axis=0)
        rec = np.zeros(xyz.shape[0], XYZIRT)
        rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        rec["intensity"] = rng.uniform(0, 255, xyz.shape[0])
        rec["ring"] = rng.integers(0, 64, xyz.shape[0])
        rec["time"] = ((np.pi - np.arctan2(xyz[:, 1], xyz[:, 0])) / (2 * np.pi) * 0.1).astype(np.float32)
        drive.append(rec)
    return drive


def ms(xs):
    return float(np.mean(xs[2:])) * 1e3


def stats(xs):
    return {"ms_median": round(float(np.median(xs)), 4), "ms_p10": round(float(np.percentile(xs, 10)), 4),
            "ms_p90": round(float(np.percentile(xs, 90)), 4), "ms_drives": [round(x, 4) for x in xs]}


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

    def new_pipeline():
        return pm.Pipeline(10.0, True, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, K, threads, False)

    def frame_drive(voxel, radius=0.0, keep=None):
        """the frame alone; voxel None: accumulation is never touched; radius 0: setMapRange is never touched"""
        pl = new_pipeline()
        if voxel is not None:
            pl.setMapAccumulation(voxel)
        if radius > 0.0:
            pl.setMapRange(radius)
        if keep is not None:
            pl.setKeepScan(True)
        ts = []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
            if keep is not None:
                keep.append((pl.registeredScan(0.0, "sensor").astype(np.float64), np.asarray(pl.currentPose()).copy()))
        info = {"rows": pl.mapSize() if voxel is not None else 0, "removed": pl.mapRemoved() if radius > 0.0 else 0}
        return ms(ts), np.asarray(pl.currentPose()), info

    if frame_only:  # (what --parent runs in the other tree: warm-up drive, then `repeats` timed ones of each leg)
        frame_drive(None)
        frame_drive(VOXEL)
        print(json.dumps({"off": [frame_drive(None)[0] for _ in range(repeats)], "map": [frame_drive(VOXEL)[0] for _ in range(repeats)]}))
        return

    def child_drive(tree):
        env = dict(os.environ, MADICP_TREE=tree, PYTHONPATH=tree)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(frames), "1", "--frame-only"], env=env, cwd=tree,
                             capture_output=True, text=True, check=True).stdout
        got = json.loads(out.strip().splitlines()[-1])
        return got["off"][0], got["map"][0]

    ctx = capi.Context.borrowed()

    def prune_legs(clouds, voxel, center, radius):
        """one prune alone, and clear + the re-fold of the last cloud, each on a freshly rebuilt map of the tool's own"""
        cids = [ctx.cloud_upload(pts) for pts, _ in clouds]
        own = ctx.map_create(voxel, 1 << 18, 1 << 24)
        out = {}
        try:
            for leg in ("prune", "clear_refold"):
                for cid, (_, T) in zip(cids, clouds):
                    ctx.map_insert_cloud(own, cid, T[:3, :3], T[:3, 3])
                out["rows"] = ctx.map_size(own)
                t1 = time.perf_counter()
                if leg == "prune":
                    out["removed"], out["kept"], _ = ctx.map_prune(own, center, radius, out["rows"])
                else:
                    ctx.map_clear(own)
                    _, out["rows_after_refold"] = ctx.map_insert_cloud(own, cids[-1], clouds[-1][1][:3, :3], clouds[-1][1][:3, 3])
                out[leg] = (time.perf_counter() - t1) * 1e3
                ctx.map_clear(own)
        finally:
            ctx.map_release(own)
            for cid in cids:
                ctx.cloud_release(cid)
        return out

    def lattice():
        i = np.arange(1 << 20)
        pts = np.stack([(i % 128) * 1.5 + 0.25, ((i // 128) % 128) * 1.5 + 0.25, (i // 16384) * 1.5 + 0.25], axis=1).astype(np.float64)
        return [(pts[k << 17:(k + 1) << 17], np.eye(4)) for k in range(8)], np.array([96.0, 96.0, 48.0]), 75.0

    frame_drive(None)  # (the first drive of a process pays for the pool's and the builder's first allocations)
    frame_drive(VOXEL, RANGE)
    if parent:
        child_drive(parent)
    res = {k: [] for k in ("off", "map", "ranged", "parent_off", "parent_map", "child_off", "child_map")}
    side = {k: [] for k in ("prune_drive", "clear_refold_drive", "prune_2p20", "clear_refold_2p20")}
    end, info, shape = {}, {}, {}
    big, big_c, big_r = lattice()
    for _ in range(repeats):
        if parent:
            a, b = child_drive(parent)
            res["parent_off"].append(a)
            res["parent_map"].append(b)
            a, b = child_drive(ROOT)
            res["child_off"].append(a)
            res["child_map"].append(b)
        t, end["off"], _ = frame_drive(None)
        res["off"].append(t)
        t, end["map"], info["map"] = frame_drive(VOXEL)
        res["map"].append(t)
        t, end["ranged"], info["ranged"] = frame_drive(VOXEL, RANGE)
        res["ranged"].append(t)
        kept = []
        frame_drive(None, keep=kept)
        got = prune_legs(kept, VOXEL, kept[-1][1][:3, 3], RANGE)
        side["prune_drive"].append(got["prune"])
        side["clear_refold_drive"].append(got["clear_refold"])
        shape["drive"] = {k: int(got[k]) for k in ("rows", "removed", "kept", "rows_after_refold")}
        got = prune_legs(big, 0.5, big_c, big_r)
        side["prune_2p20"].append(got["prune"])
        side["clear_refold_2p20"].append(got["clear_refold"])
        shape["2p20"] = {k: int(got[k]) for k in ("rows", "removed", "kept", "rows_after_refold")}
    for k in ("map", "ranged"):
        assert np.array_equal(end["off"].view(np.uint64), end[k].view(np.uint64)), "the option changed the pose"

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_bit_equal": True, "voxel": VOXEL, "range": RANGE,
           "frame_off": stats(res["off"]), "frame_map_no_range": dict(stats(res["map"]), map_rows=int(info["map"]["rows"])),
           "frame_map_ranged": dict(stats(res["ranged"]), map_rows=int(info["ranged"]["rows"]), rows_removed=int(info["ranged"]["removed"]))}
    if parent:
        out["frame_off_parent_commit"] = stats(res["parent_off"])
        out["frame_map_parent_commit"] = stats(res["parent_map"])
        out["frame_off_this_tree_child"] = stats(res["child_off"])
        out["frame_map_this_tree_child"] = stats(res["child_map"])
    for k, v in side.items():
        out[k] = stats(v)
    out["prune_shapes"] = shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
