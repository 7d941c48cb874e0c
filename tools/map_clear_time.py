"""What free-space clearing of the voxel map costs: the frame with Pipeline.setMapClearing off against the parent commit's frame, the
frame with clearing on against the same map without it, one Context.map_clear_rays alone, and — for scale — the host twin on the
same inputs, which is what a consumer of mapNewRows() does today.  One process.

  python tools/map_clear_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/map_clear_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)

The scans are the 120 k-point synthetic drive of tools/map_prune_time.py (22-byte XYZIRT records, 1 m per frame), fed to default
Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive, `repeats` drives each:

  (i)   off         the frame — pl.computeRecordsStamped(...) alone, a host clock around the call (it returns after the result has
                    been read back: a synchronised time) — of a Pipeline with accumulation off.
        parent_off  --parent TREE: the same frame of ANOTHER built tree of this project (the parent commit's), this file run with
                    --frame-only in a child process per drive, interleaved with the legs above — the same box, the same session.
                    --frame-only touches nothing the parent lacks.
        child_off   ... and of THIS tree run the same way, in a child process per drive: the like-for-like partner of parent_off.
  (ii)  map / cleared   the frame of a Pipeline with setMapAccumulation(0.2), and of one with setMapClearing(True) as well: the
                    difference is the price per frame (the cleared map is also smaller: its folds see fewer rows).  All legs must
                    end on the same pose bit for bit (asserted).
  (iii) clear_rays  one Context.map_clear_rays alone on a map of the tool's own — the drive's 0.2 m map (every frame's compensated
                    scan folded at its pose, nothing cleared), the rays of the last scan at its pose.  Each repeat rebuilds the map
                    first, outside the clock.
  (iv)  host_twin   capi.host_map_clear_rays on the same map and rays: two hash sets and one pass on one core.

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mad_icp_amd import capi  # noqa: E402
from map_prune_time import B_MAX, B_MIN, B_RATIO, HI, LO, RHO_KER, K, make_drive, ms, stats  # noqa: E402

VOXEL, MARGIN = 0.2, 0.0


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

    def frame_drive(voxel, clearing=False, keep=None):
        """the frame alone; voxel None: accumulation is never touched; clearing False: setMapClearing is never touched"""
        pl = pm.Pipeline(10.0, True, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, K, threads, False)
        if voxel is not None:
            pl.setMapAccumulation(voxel)
        if clearing:
            pl.setMapClearing(True, MARGIN)
        if keep is not None:
            pl.setKeepScan(True)
        ts = []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
            if keep is not None:
                keep.append((pl.registeredScan(0.0, "sensor").astype(np.float64), np.asarray(pl.currentPose()).copy()))
        info = {"rows": pl.mapSize() if voxel is not None else 0, "removed": pl.mapRemoved() if clearing else 0}
        return ms(ts), np.asarray(pl.currentPose()), info

    if frame_only:  # (what --parent runs in the other tree: warm-up drives, then `repeats` timed ones)
        frame_drive(None)
        frame_drive(None)
        print(json.dumps({"off": [frame_drive(None)[0] for _ in range(repeats)]}))
        return

    def child_drive(tree):
        env = dict(os.environ, MADICP_TREE=tree, PYTHONPATH=tree)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(frames), "1", "--frame-only"], env=env, cwd=tree,
                             capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])["off"][0]

    ctx = capi.Context.borrowed()

    def clear_legs(clouds):
        """one clearing alone by the rays of the last cloud, on the device and in the host twin, each on a freshly built map"""
        rays, T = clouds[-1]
        R, t = T[:3, :3], T[:3, 3]
        out = {}
        cids = [ctx.cloud_upload(pts) for pts, _ in clouds]
        own = ctx.map_create(VOXEL, 1 << 18, 1 << 24)
        try:
            for cid, (_, Tk) in zip(cids, clouds):
                ctx.map_insert_cloud(own, cid, Tk[:3, :3], Tk[:3, 3])
            out["rows"] = ctx.map_size(own)
            t1 = time.perf_counter()
            out["removed"], out["kept"], _ = ctx.map_clear_rays(own, cids[-1], R, t, (0.0, 0.0, 0.0), MARGIN, out["rows"])
            out["clear_rays"] = (time.perf_counter() - t1) * 1e3
            rows = ctx.map_download_f32(own)
        finally:
            ctx.map_release(own)
            for cid in cids:
                ctx.cloud_release(cid)
        h = capi.host_map_create(VOXEL, 1 << 18, 1 << 24)
        try:
            for pts, Tk in clouds:
                capi.host_map_insert(h, pts, Tk[:3, :3], Tk[:3, 3])
            t1 = time.perf_counter()
            got = capi.host_map_clear_rays(h, rays, R, t, (0.0, 0.0, 0.0), MARGIN, out["rows"])
            out["host_twin"] = (time.perf_counter() - t1) * 1e3
            assert got[:2] == (out["removed"], out["kept"]) and capi.host_map_download_f32(h).tobytes() == rows.tobytes(), "device and twin differ"
        finally:
            capi.host_map_destroy(h)
        return out

    frame_drive(None)  # (the first drive of a process pays for the pool's and the builder's first allocations)
    frame_drive(VOXEL, True)
    if parent:
        child_drive(parent)
    res = {k: [] for k in ("off", "map", "cleared", "parent_off", "child_off")}
    side = {k: [] for k in ("clear_rays", "host_twin")}
    end, info, shape = {}, {}, {}
    for r in range(repeats):
        print("map_clear_time: drive set %d of %d" % (r + 1, repeats), file=sys.stderr, flush=True)
        if parent:
            res["parent_off"].append(child_drive(parent))
            res["child_off"].append(child_drive(ROOT))
        t, end["off"], _ = frame_drive(None)
        res["off"].append(t)
        t, end["map"], info["map"] = frame_drive(VOXEL)
        res["map"].append(t)
        t, end["cleared"], info["cleared"] = frame_drive(VOXEL, True)
        res["cleared"].append(t)
        kept = []
        frame_drive(None, keep=kept)
        got = clear_legs(kept)
        for k in side:
            side[k].append(got[k])
        shape = {k: int(got[k]) for k in ("rows", "removed", "kept")}
        shape["rays"] = int(kept[-1][0].shape[0])
    for k in ("map", "cleared"):
        assert np.array_equal(end["off"].view(np.uint64), end[k].view(np.uint64)), "the option changed the pose"

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_bit_equal": True, "voxel": VOXEL, "margin": MARGIN,
           "frame_off": stats(res["off"]), "frame_map_no_clearing": dict(stats(res["map"]), map_rows=int(info["map"]["rows"])),
           "frame_map_cleared": dict(stats(res["cleared"]), map_rows=int(info["cleared"]["rows"]), rows_removed=int(info["cleared"]["removed"]))}
    if parent:
        out["frame_off_parent_commit"] = stats(res["parent_off"])
        out["frame_off_this_tree_child"] = stats(res["child_off"])
    for k, v in side.items():
        out[k] = stats(v)
    out["clear_shape"] = shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
