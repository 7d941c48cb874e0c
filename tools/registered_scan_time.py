"""What the registered scan out costs: the frame with Pipeline.setKeepScan on against off, and registeredScan() against what a
caller could do before it existed, one process.

  python tools/registered_scan_time.py [frames=16] [repeats=5]

The scans are the 120 k-point synthetic drive of tools/records_stamped_frame_time.py (22-byte XYZIRT records, about 3 % outside the
range filter), fed to default Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive
by drive, `repeats` drives each:

  (a) off / on   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call (it returns after the result has been
                 read back: a synchronised time) — of a Pipeline with the option off and of one with it on.  The off frame is the
                 frame as it was before the option existed; the on frame differs by one pool buffer that is not given back.  Both
                 must end on the same pose bit for bit (asserted).
  (b) scan_v     pl.registeredScan(v, "map") for v = 0, 0.2, 0.5 after every frame of an on drive, OUTSIDE the frame's timed region;
      today_v    what a caller can do without it: madicp_cloud_download of a resident cloud of the same size (float64: twice the
                 bytes) + the rule in numpy on the host (pose, voxel keys, np.unique for the first index per key, float32).  The
                 cloud is the frame's own compensated scan; row counts of the two are asserted equal.

The first two frames of a drive (no deskew yet, first allocations) are left out; per drive the mean over frames, then median / p10 /
p90 over the drives.  Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mad_icp_amd import capi, synth  # noqa: E402

B_MAX, B_MIN, RHO_KER, B_RATIO, K = 0.2, 0.1, 0.1, 0.02, 16
LO, HI = 0.7, 120.0
VOXELS = (0.0, 0.2, 0.5)
XYZIRT = np.dtype(dict(names=["x", "y", "z", "intensity", "ring", "time"], formats=["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"],
                       offsets=[0, 4, 8, 12, 16, 18], itemsize=22))


def numpy_export(p, T, voxel):
    """the export rule of include/madicp_hip.h on the host (tests/cloud_export_ref.py)"""
    R, t = T[:3, :3], T[:3, 3]
    q = np.empty_like(p)
    for i in range(3):
        q[:, i] = t[i] + (R[i, 0] * p[:, 0] + (R[i, 1] * p[:, 1] + R[i, 2] * p[:, 2]))
    if voxel == 0:
        return q.astype(np.float32)
    f = np.floor(q / voxel)
    idx = np.nonzero(np.all((f >= -1048576.0) & (f < 1048576.0), axis=1))[0]
    k = f[idx].astype(np.int64) + 1048576
    _, first = np.unique(k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42), return_index=True)
    return q[np.sort(idx[first])].astype(np.float32)


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
        rec["time"] = ((np.pi - np.arctan2(xyz[:, 1], xyz[:, 0])) / (2 * np.pi) * 0.1).astype(np.float32)
        drive.append(rec)
    threads = min(os.cpu_count() or 1, 16)
    ctx = capi.Context.borrowed()
    rows = {}

    def one_drive(keep, export):
        pl = pm.Pipeline(10.0, True, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, K, threads, False)
        pl.setKeepScan(keep)
        ts = []
        scan = {v: [] for v in VOXELS}
        today = {v: [] for v in VOXELS}
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
            if not export:
                continue
            T = np.asarray(pl.currentPose())
            got = {}
            for v in VOXELS:
                t1 = time.perf_counter()
                got[v] = pl.registeredScan(v, "map")
                scan[v].append(time.perf_counter() - t1)
            # today's route on a resident cloud of the same content (the frame's compensated scan, widened: what the device holds)
            cid = ctx.cloud_upload(pl.registeredScan(0.0, "sensor").astype(np.float64))
            for v in VOXELS:
                t1 = time.perf_counter()
                out = numpy_export(ctx.cloud_download(cid), T, v)
                today[v].append(time.perf_counter() - t1)
                assert abs(out.shape[0] - got[v].shape[0]) <= got[v].shape[0] // 100, (i, v, out.shape, got[v].shape)
                rows[v] = int(got[v].shape[0])
            ctx.cloud_release(cid)
        ms = lambda xs: float(np.mean(xs[2:])) * 1e3  # noqa: E731
        return ms(ts), {v: ms(scan[v]) for v in VOXELS} if export else None, {v: ms(today[v]) for v in VOXELS} if export else None, \
            np.asarray(pl.currentPose())

    for keep in (False, True):  # (the first drive of a process pays for the pool's and the builder's first allocations)
        one_drive(keep, keep)
    res = {"off": [], "on": []}
    scan = {v: [] for v in VOXELS}
    today = {v: [] for v in VOXELS}
    end = {}
    for _ in range(repeats):
        for name, keep in (("off", False), ("on", True)):
            ms, _, _, pose = one_drive(keep, False)
            res[name].append(ms)
            end[name] = pose
        _, s, t, _ = one_drive(True, True)
        for v in VOXELS:
            scan[v].append(s[v])
            today[v].append(t[v])
    assert np.array_equal(end["off"].view(np.uint64), end["on"].view(np.uint64)), "the option changed the pose"

    def stats(xs):
        return {"ms_median": round(float(np.median(xs)), 4), "ms_p10": round(float(np.percentile(xs, 10)), 4),
                "ms_p90": round(float(np.percentile(xs, 90)), 4), "ms_drives": [round(x, 4) for x in xs]}

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_caller": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_bit_equal": True, "frame_off": stats(res["off"]), "frame_on": stats(res["on"])}
    for v in VOXELS:
        out["registered_scan_%g" % v] = dict(stats(scan[v]), rows=rows[v])
        out["download_plus_numpy_%g" % v] = stats(today[v])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
