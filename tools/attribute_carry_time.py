"""What carrying a per-point attribute costs: the frame without one against the parent commit's, the frame with the attribute carried
to the retained scan and into the map, and the read-outs with and without the column, one process.

  python tools/attribute_carry_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/attribute_carry_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)

The scans are the 120 k-point synthetic drive of tools/map_accumulate_time.py (22-byte XYZIRT records, about 3 % outside the range
filter), fed to default Pipelines (deskew = True, device front-end) through computeRecordsStamped; the attribute is the records'
float32 `intensity`.  Timed, interleaved drive by drive, `repeats` drives each — the frame is pl.computeRecordsStamped(...) alone, a
host clock around the call (it returns after the result has been read back: a synchronised time):

  (a) parent       --parent TREE: the frame of ANOTHER built tree of this project (the parent commit's), the same drive through this
                   file run with --frame-only in a child process per drive, interleaved with the legs below — the same box, the same
                   session.  --frame-only touches nothing the parent lacks.
  (b) plain        this tree, no attribute asked for anywhere.
  (c) keep_attr    attribute = "intensity", setKeepScan(True): the column rides through ingest and deskew and stays with the scan.
      keep_plain   setKeepScan(True) without the attribute: what (c) is to be compared with.
  (d) map_attr     attribute = "intensity", setMapAccumulation(0.2, with_attribute=True): the column is folded into the map.
      map_plain    setMapAccumulation(0.2) without the attribute: what (d) is to be compared with.
  scan / scan_attr     pl.registeredScan(0.2, "map") and the same with with_attribute=True, after every frame, outside the frame.
  fetch / fetch_attr   pl.mapCloud(the size before the frame) and the same with with_attribute=True.

All legs must end on the same pose bit for bit (asserted).  The first two frames of a drive (no deskew yet, first allocations) are
left out; per drive the mean over frames, then median / p10 / p90 over the drives.  Prints one JSON line.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("MADICP_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mad_icp_amd import synth  # noqa: E402

B_MAX, B_MIN, RHO_KER, B_RATIO, K = 0.2, 0.1, 0.1, 0.02, 16
LO, HI = 0.7, 120.0
VOXEL = 0.2
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

    def frame_drive(attr=False, keep=False, voxel=None, readouts=None):
        """the frame alone; with `readouts` (a dict of lists) the scan / map read-outs after every frame, outside the frame"""
        pl = new_pipeline()
        if keep:
            pl.setKeepScan(True)
        if voxel is not None:
            pl.setMapAccumulation(voxel, with_attribute=True) if attr else pl.setMapAccumulation(voxel)
        ts = []
        local = {k: [] for k in (readouts or {})}
        for i, rec in enumerate(drive):
            before = pl.mapSize() if voxel is not None else 0
            t1 = time.perf_counter()
            if attr:
                pl.computeRecordsStamped(0.1 * i, rec, LO, HI, attribute="intensity")
            else:
                pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
            if readouts is not None:
                t1 = time.perf_counter()
                rows = pl.registeredScan(VOXEL, "map")
                local["scan"].append(time.perf_counter() - t1)
                t1 = time.perf_counter()
                rows_a, words = pl.registeredScan(VOXEL, "map", with_attribute=True)
                local["scan_attr"].append(time.perf_counter() - t1)
                assert rows_a.tobytes() == rows.tobytes() and words.dtype == np.float32 and words.shape == (rows.shape[0],)
                t1 = time.perf_counter()
                new_rows = pl.mapCloud(before)
                local["fetch"].append(time.perf_counter() - t1)
                t1 = time.perf_counter()
                new_rows_a, words = pl.mapCloud(before, with_attribute=True)
                local["fetch_attr"].append(time.perf_counter() - t1)
                assert new_rows_a.tobytes() == new_rows.tobytes() and words.shape == (new_rows.shape[0],)
        for k in local:
            readouts[k].append(ms(local[k]))
        return ms(ts), np.asarray(pl.currentPose())

    if frame_only:  # (what --parent runs in the other tree: warm-up drive, then `repeats` timed ones)
        frame_drive()
        print(json.dumps({"frame_ms_drives": [frame_drive()[0] for _ in range(repeats)]}))
        return

    def parent_drive():
        env = dict(os.environ, MADICP_TREE=parent, PYTHONPATH=parent)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(frames), "1", "--frame-only"], env=env, cwd=parent,
                             capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])["frame_ms_drives"][0]

    legs = {"plain": dict(), "keep_plain": dict(keep=True), "keep_attr": dict(attr=True, keep=True), "map_plain": dict(voxel=VOXEL),
            "map_attr": dict(attr=True, voxel=VOXEL)}
    frame_drive()  # (the first drive of a process pays for the pool's and the builder's first allocations)
    frame_drive(attr=True, keep=True, voxel=VOXEL)
    if parent:
        parent_drive()
    res = {k: [] for k in list(legs) + ["parent"]}
    readouts = {"scan": [], "scan_attr": [], "fetch": [], "fetch_attr": []}
    end = {}
    for _ in range(repeats):
        if parent:
            res["parent"].append(parent_drive())
        for name, kw in legs.items():
            t, end[name] = frame_drive(**kw)
            res[name].append(t)
        frame_drive(attr=True, keep=True, voxel=VOXEL, readouts=readouts)
    for name in legs:
        assert np.array_equal(end["plain"].view(np.uint64), end[name].view(np.uint64)), "the attribute changed the pose: " + name

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_bit_equal": True, "voxel": VOXEL}
    if parent:
        out["frame_parent_commit"] = stats(res["parent"])
    for name in legs:
        out["frame_" + name] = stats(res[name])
    for name, xs in readouts.items():
        out[name] = stats(xs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
