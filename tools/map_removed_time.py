"""What reporting the voxel map's removals costs: the frame with Pipeline.setMapTrackRemoved off against the parent commit's frame,
the frame of a cleared and ranged map with tracking off against on, one Context.map_prune and one Context.map_clear_rays alone
with tracking off against on, one poll against what a consumer has to do without the log, and mapNewRows(with_attribute=True)
through the one-wait download against the two-wait path.

  python tools/map_removed_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/map_removed_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)

The scans are the 120 k-point synthetic drive of tools/map_prune_time.py (22-byte XYZIRT records, 1 m per frame), fed to default
Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive, `repeats` drives each:

  (i)   parent_off / child_off   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call, accumulation off — of
                    ANOTHER built tree of this project (--parent TREE: the parent commit's) and of THIS tree, each in a child
                    process per drive (this file with --frame-only, which touches nothing the parent lacks): child against child.
  (ii)  track_off / track_on   the frame of a Pipeline with setMapAccumulation(0.2), setMapClearing(True) and setMapRange(20), with
                    setMapTrackRemoved off and on.  A consumer polls after every frame, outside the frame's clock.  All legs must
                    end on the same pose and the same map, bit for bit (asserted).
  (iv)  poll_log / poll_whole   that consumer's poll, timed on its own.  With the log: mapRemovedRows() + mapNewRows(with_keys=True).
                    Without it, what learns of removals today: mapCloud(0) of the whole map and a set difference of the rows' bytes
                    against the previous copy on the host.
  (iii) prune / clear_rays, each _off and _on   one Context.map_prune (a sphere of 20 m about the last pose) and one
                    Context.map_clear_rays (the rays of the last scan) alone on the drive's 0.2 m map rebuilt outside the clock, the
                    watermark at the map's rows — every removed row is logged; the first logging removal of a map also allocates
                    the log.
  (v)   new_rows_attr_one_wait / _two_waits   per frame, the new rows and their words of an append-only 0.2 m map with the attribute
                    column: mapNewRows(with_attribute=True) (madicp_map_download_rows) against mapCloud(first_row,
                    with_attribute=True) (madicp_map_download_f32, then madicp_map_download_attr: the path mapNewRows took before).

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
from map_prune_time import B_MAX, B_MIN, B_RATIO, HI, LO, RANGE, RHO_KER, VOXEL, K, make_drive, ms, stats  # noqa: E402

MARGIN = 0.0


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

    def mapped_drive(track):
        """(ii) and (iv): the frame and the consumer's poll, each under its own clock"""
        pl = pipeline()
        pl.setMapAccumulation(VOXEL)
        pl.setMapClearing(True, MARGIN)
        pl.setMapRange(RANGE)
        if track:
            pl.setMapTrackRemoved(True)
        ts, polls, held, logged = [], [], set(), 0
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            t2 = time.perf_counter()
            if track:
                gone_keys, _ = pl.mapRemovedRows()
                rows, keys = pl.mapNewRows(with_keys=True)
                logged += gone_keys.shape[0]
            else:
                whole = pl.mapCloud(0)
                now = set(map(bytes, whole.view(np.uint8).reshape(-1, 12)))
                gone, new = held - now, now - held  # noqa: F841  (what the consumer needs: the rows that left, the rows to add)
                held = now
                pl.mapNewRows()  # (the cursor moves as it does in the other leg: the watermarks are the same)
            t3 = time.perf_counter()
            ts.append(t2 - t1)
            polls.append(t3 - t2)
        info = {"rows": pl.mapSize(), "removed": pl.mapRemoved(), "logged": logged}
        return ms(ts), ms(polls), np.asarray(pl.currentPose()), pl.mapCloud(0).tobytes(), info

    def attr_drive(one_wait):
        """(v): the new rows with their words, per frame, through one wait or two"""
        pl = pipeline()
        pl.setMapAccumulation(VOXEL, with_attribute=True)
        ts, first = [], 0
        for i, rec in enumerate(drive):
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI, attribute="intensity")
            t1 = time.perf_counter()
            if one_wait:
                rows, _ = pl.mapNewRows(with_attribute=True)
            else:
                rows, _ = pl.mapCloud(first, with_attribute=True)
            ts.append(time.perf_counter() - t1)
            first += rows.shape[0]
        assert first == pl.mapSize()
        return ms(ts), first

    ctx = capi.Context.borrowed()

    def removal_legs(clouds, track):
        """(iii): one prune and one clearing alone, each on a freshly built map, the watermark at its rows"""
        rays, T = clouds[-1]
        R, t = T[:3, :3], T[:3, 3]
        out = {}
        cids = [ctx.cloud_upload(pts) for pts, _ in clouds]
        try:
            for what in ("prune", "clear_rays"):
                own = ctx.map_create(VOXEL, 1 << 18, 1 << 24)
                try:
                    if track:
                        ctx.map_track_removed(own, True)
                    for cid, (_, Tk) in zip(cids, clouds):
                        ctx.map_insert_cloud(own, cid, Tk[:3, :3], Tk[:3, 3])
                    rows = ctx.map_size(own)
                    t1 = time.perf_counter()
                    if what == "prune":
                        removed, _, mark = ctx.map_prune(own, t, RANGE, rows)
                    else:
                        removed, _, mark = ctx.map_clear_rays(own, cids[-1], R, t, (0.0, 0.0, 0.0), MARGIN, rows)
                    out[what] = (time.perf_counter() - t1) * 1e3
                    out[what + "_shape"] = {"rows": rows, "removed": removed}
                    assert ctx.map_removed_count(own) == (removed if track else 0) and mark == rows - removed
                    out[what + "_map"] = ctx.map_download_f32(own).tobytes()
                finally:
                    ctx.map_release(own)
        finally:
            for cid in cids:
                ctx.cloud_release(cid)
        return out

    plain_drive()  # (the first drive of a process pays for the pool's and the builder's first allocations)
    mapped_drive(True)
    if parent:
        child_drive(parent)
    res = {k: [] for k in ("parent_off", "child_off", "track_off", "track_on", "poll_whole", "poll_log", "new_rows_attr_one_wait",
                           "new_rows_attr_two_waits", "prune_off", "prune_on", "clear_rays_off", "clear_rays_on")}
    end, info, shape = {}, {}, {}
    for r in range(repeats):
        print("map_removed_time: drive set %d of %d" % (r + 1, repeats), file=sys.stderr, flush=True)
        if parent:
            res["parent_off"].append(child_drive(parent))
            res["child_off"].append(child_drive(ROOT))
        for track, leg, poll in ((False, "track_off", "poll_whole"), (True, "track_on", "poll_log")):
            t, p, pose, rows, info[leg] = mapped_drive(track)
            res[leg].append(t)
            res[poll].append(p)
            end[leg] = (pose.tobytes(), rows)
        assert end["track_off"] == end["track_on"], "tracking changed the pose or the map"
        for one_wait, leg in ((True, "new_rows_attr_one_wait"), (False, "new_rows_attr_two_waits")):
            t, info[leg] = attr_drive(one_wait)
            res[leg].append(t)
        kept = []
        plain_drive(keep=kept)
        legs = {track: removal_legs(kept, track) for track in (False, True)}
        for what in ("prune", "clear_rays"):
            assert legs[False][what + "_map"] == legs[True][what + "_map"], "tracking changed the map"
            res[what + "_off"].append(legs[False][what])
            res[what + "_on"].append(legs[True][what])
            shape[what] = legs[True][what + "_shape"]

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_and_maps_bit_equal": True, "voxel": VOXEL, "margin": MARGIN, "range": RANGE}
    for k, v in res.items():
        if v:
            out[k] = stats(v)
    out["frame_map"] = {k: {kk: int(vv) for kk, vv in info[k].items()} for k in ("track_off", "track_on")}
    out["attr_map_rows"] = int(info["new_rows_attr_one_wait"])
    out["removal_shape"] = shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
