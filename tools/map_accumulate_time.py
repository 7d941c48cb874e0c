"""What map accumulation costs: the frame with Pipeline.setMapAccumulation off against on, one fold, the per-frame fetch of the new
rows, and what a consumer does today for the same map, one process.

  python tools/map_accumulate_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/map_accumulate_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)

The scans are the 120 k-point synthetic drive of tools/registered_scan_time.py (22-byte XYZIRT records, about 3 % outside the range
filter), fed to default Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by
drive, `repeats` drives each:

  (a) off / on_v   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call (it returns after the result has been
                   read back: a synchronised time) — of a Pipeline with the option off and of one with setMapAccumulation(v),
                   v = 0.2, 0.5.  The on frame contains the fold.  All must end on the same pose bit for bit (asserted).
      parent       --parent TREE: the off frame of ANOTHER built tree of this project (the parent commit's), the same drive through
                   this file run with --frame-only in a child process per drive, interleaved with the legs above — the same box, the
                   same session.  --frame-only touches nothing the parent lacks.
  (b) fold_v       Context.map_insert_cloud of the frame's own compensated scan (kept with setKeepScan, folded at the frame's pose into
                   a map of the tool's own) after every frame of a drive, OUTSIDE the frame's timed region: one fold alone.
  (c) fetch_v      pl.mapCloud(first_row = the size before the frame) after every frame: the rows the frame added.
  (d) today_v      what a consumer does today for the same map: pl.registeredScan(v, "map") + a host-side merge — the voxel keys of
                   the returned float rows in numpy, looked up in a Python set, the new ones appended.  (Its keys come from the stored
                   floats, so its map can differ from (a)'s by points within half a float ulp of a cell face; sizes are reported.)

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
VOXELS = (0.2, 0.5)
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


def float_keys(rows, voxel):
    """the voxel keys a host-side consumer computes from the float rows it was given"""
    f = np.floor(rows.astype(np.float64) / voxel).astype(np.int64) + 1048576
    return f[:, 0] | (f[:, 1] << 21) | (f[:, 2] << 42)


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

    def frame_drive(voxel):
        """the frame alone; voxel None: the option is never touched"""
        pl = new_pipeline()
        if voxel is not None:
            pl.setMapAccumulation(voxel)
        ts = []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
        return ms(ts), np.asarray(pl.currentPose()), (pl.mapSize() if voxel is not None else 0)

    if frame_only:  # (what --parent runs in the other tree: warm-up drive, then `repeats` timed ones)
        frame_drive(None)
        print(json.dumps({"frame_ms_drives": [frame_drive(None)[0] for _ in range(repeats)]}))
        return

    def parent_drive():
        env = dict(os.environ, MADICP_TREE=parent, PYTHONPATH=parent)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(frames), "1", "--frame-only"], env=env, cwd=parent,
                             capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])["frame_ms_drives"][0]

    ctx = capi.Context.borrowed()

    def side_drive(voxel):
        """(b) one fold alone, (c) the fetch of the new rows, (d) today's route — each outside the frame"""
        pl, today_pl = new_pipeline(), new_pipeline()
        pl.setMapAccumulation(voxel)
        pl.setKeepScan(True)
        today_pl.setKeepScan(True)
        own = ctx.map_create(voxel, 1 << 18, 1 << 24)
        seen, today_rows = set(), 0
        fold, fetch, today = [], [], []
        for i, rec in enumerate(drive):
            before = pl.mapSize()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            today_pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            T = np.asarray(pl.currentPose())
            t1 = time.perf_counter()
            new_rows = pl.mapCloud(before)
            fetch.append(time.perf_counter() - t1)
            assert new_rows.shape[0] == pl.mapSize() - before
            cid = ctx.cloud_upload(pl.registeredScan(0.0, "sensor").astype(np.float64))
            t1 = time.perf_counter()
            ctx.map_insert_cloud(own, cid, T[:3, :3], T[:3, 3])
            fold.append(time.perf_counter() - t1)
            ctx.cloud_release(cid)
            t1 = time.perf_counter()
            scan = today_pl.registeredScan(voxel, "map")
            keys = float_keys(scan, voxel).tolist()
            fresh = [j for j, k in enumerate(keys) if k not in seen]
            seen.update(keys[j] for j in fresh)
            today_rows += scan[fresh].shape[0]
            today.append(time.perf_counter() - t1)
        size = pl.mapSize()
        # (the tool's own map is fed the float32 scan widened again: a point within half a float ulp of a cell face can change cells)
        assert abs(ctx.map_size(own) - size) <= size // 100, (ctx.map_size(own), size)
        ctx.map_release(own)
        return ms(fold), ms(fetch), ms(today), size, today_rows

    frame_drive(None)  # (the first drive of a process pays for the pool's and the builder's first allocations)
    frame_drive(VOXELS[0])
    if parent:
        parent_drive()
    res = {"off": [], "parent": []}
    res.update({"on_%g" % v: [] for v in VOXELS})
    side = {v: {"fold": [], "fetch": [], "today": []} for v in VOXELS}
    end, sizes = {}, {}
    for _ in range(repeats):
        if parent:
            res["parent"].append(parent_drive())
        t, end["off"], _ = frame_drive(None)
        res["off"].append(t)
        for v in VOXELS:
            t, end[v], sizes[v] = frame_drive(v)
            res["on_%g" % v].append(t)
        for v in VOXELS:
            f, g, d, size, today_rows = side_drive(v)
            side[v]["fold"].append(f)
            side[v]["fetch"].append(g)
            side[v]["today"].append(d)
            assert size == sizes[v]
            sizes["today_%g" % v] = today_rows
    for v in VOXELS:
        assert np.array_equal(end["off"].view(np.uint64), end[v].view(np.uint64)), "the option changed the pose"

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_bit_equal": True, "frame_off": stats(res["off"])}
    if parent:
        out["frame_parent_commit"] = stats(res["parent"])
    for v in VOXELS:
        out["frame_on_%g" % v] = dict(stats(res["on_%g" % v]), map_rows=int(sizes[v]))
        out["fold_%g" % v] = stats(side[v]["fold"])
        out["fetch_new_rows_%g" % v] = stats(side[v]["fetch"])
        out["registered_scan_plus_host_merge_%g" % v] = dict(stats(side[v]["today"]), map_rows=int(sizes["today_%g" % v]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
