"""Frame time of a stamped-deskew drive fed RAW RECORDS against the same drive fed host-prepared arrays, one process.

  python tools/records_stamped_frame_time.py [frames=16] [repeats=5]

The scans are the 120 k-point synthetic drive of tools/stamped_frame_time.py as a driver would deliver them: float32 x / y / z,
an intensity, a ring and a float32 per-point time, packed into 22-byte XYZIRT records (every record at another alignment), with
about 3 % of the records outside the range filter.  Three things are timed, interleaved drive by drive, `repeats` drives each:

  records   pl.computeRecordsStamped(stamp, records, lo, hi)   the buffer as it is: filter, compaction and the stamps on the device
  arrays    pl.compute(stamp, cloud, stamps)                   the same build fed what `prepare` made (made OUTSIDE the timed region)
  prepare   the host preparation the arrays caller needs first: numpy unpack of the unaligned fields, range filter, widening to
            float64, min / max of the times and normalisation — per frame, on its own

Both callers are default Pipelines with deskew = True on the device front-end and must end on the same pose bit for bit (asserted).
compute() returns after the registration's result has been read back, so a host clock around it is a synchronised time.  The
first two frames of a drive (no deskew yet, first allocations) are left out; per drive the mean over frames, then median / p10 /
p90 over the drives.  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mad_icp_amd import synth  # noqa: E402

B_MAX, B_MIN, RHO_KER, B_RATIO, K = 0.2, 0.1, 0.1, 0.02, 16
LO, HI = 0.7, 120.0
XYZIRT = np.dtype(dict(names=["x", "y", "z", "intensity", "ring", "time"], formats=["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"],
                       offsets=[0, 4, 8, 12, 16, 18], itemsize=22))


def prepare(rec):
    """what a caller of compute(stamp, cloud, stamps) does on the host with a driver's buffer"""
    x, y, z = rec["x"], rec["y"], rec["z"]
    with np.errstate(invalid="ignore", over="ignore"):
        nrm = np.sqrt(x * x + (y * y + z * z)).astype(np.float64)
        keep = ~((nrm < LO) | (nrm > HI) | np.isnan(x) | np.isnan(y) | np.isnan(z))
    pts = np.empty((int(keep.sum()), 3))
    pts[:, 0], pts[:, 1], pts[:, 2] = x[keep], y[keep], z[keep]
    t = rec["time"].astype(np.float64)
    fin = t[np.isfinite(t)]
    t0, t1 = fin.min() + 0.0, fin.max() + 0.0
    return pts, np.ascontiguousarray(((t - t0) / (t1 - t0))[keep])


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    from mad_icp.src.pybind import pypeline as pm

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
        # the head starts at +pi and turns clockwise over 0.1 s: the model the azimuth path assumes
        rec["time"] = ((np.pi - np.arctan2(xyz[:, 1], xyz[:, 0])) / (2 * np.pi) * 0.1).astype(np.float32)
        drive.append(rec)
    prepared = [prepare(rec) for rec in drive]
    threads = min(os.cpu_count() or 1, 16)

    def one_drive(kind):
        if kind == "prepare":
            ts = []
            for rec in drive:
                t1 = time.perf_counter()
                prepare(rec)
                ts.append(time.perf_counter() - t1)
            return float(np.mean(ts[2:])) * 1e3, 0.0, None
        pl = pm.Pipeline(10.0, True, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, K, threads, False)
        ts, build = [], []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            if kind == "records":
                pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            else:
                pl.compute(0.1 * i, prepared[i][0], prepared[i][1])
            ts.append(time.perf_counter() - t1)
            build.append(pl.lastBuildMs())
        return float(np.mean(ts[2:])) * 1e3, float(np.mean(build[2:])), np.asarray(pl.currentPose())

    kinds = ("records", "arrays", "prepare")
    for kind in kinds:  # (the first drive of a process pays for the pool's and the builder's first allocations)
        one_drive(kind)
    res = {k: [] for k in kinds}
    front = {k: [] for k in kinds}
    end = {}
    for _ in range(repeats):
        for kind in kinds:
            ms, b, pose = one_drive(kind)
            res[kind].append(ms)
            front[kind].append(b)
            end[kind] = pose
    assert np.array_equal(end["records"].view(np.uint64), end["arrays"].view(np.uint64)), "the two callers ended on different poses"
    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_caller": repeats,
           "records_per_scan": int(drive[0].shape[0]), "points_per_scan": int(prepared[0][0].shape[0]), "point_step": XYZIRT.itemsize,
           "host_threads": threads, "end_poses_bit_equal": True}
    for kind in kinds:
        out[kind] = {"ms_per_frame_median": round(float(np.median(res[kind])), 4),
                     "ms_per_frame_p10": round(float(np.percentile(res[kind], 10)), 4),
                     "ms_per_frame_p90": round(float(np.percentile(res[kind], 90)), 4),
                     "ms_per_frame_drives": [round(x, 4) for x in res[kind]]}
        if kind != "prepare":
            out[kind]["front_end_ms_median"] = round(float(np.median(front[kind])), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
