"""What registering a scan against the voxel map's surfels costs: the frame with every new option off against the parent commit's
frame, the frame of a 0.2 m moments map without and with setMapAlignment, and one Context.map_register_cloud alone — one
linearisation and a 5-round registration, both reaches — against the host twin on the same inputs.

  python tools/map_register_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/map_register_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)
  python tools/map_register_time.py [frames] --register-only                 (the alone legs once more, in a loop: for a kernel trace)

The scans are the 120 k-point synthetic drive of tools/map_prune_time.py (22-byte XYZIRT records, 1 m per frame), fed to default
Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive, `repeats` drives each:

  (i)   parent_off / child_off   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call, accumulation off — of
                    ANOTHER built tree of this project (--parent TREE: the parent commit's) and of THIS tree, each in a child
                    process per drive (this file with --frame-only, which touches nothing the parent lacks): child against child.
  (ii)  align_off / align_on   the frame of a Pipeline with setMapAccumulation(0.2, moments=2^20), without and with
                    setMapAlignment(True, 5, ...).  Both legs must end on the same pose and the same map rows, bit for bit (asserted).
  (iii) lin_r{0,1} / reg5_r{0,1}   one Context.map_register_cloud of the last scan (resident), from its pose offset by a few centimetres
                    and about a degree, against the 0.2 m moments map of the whole drive, the map built outside the clock: iterations
                    0 (no per-point column) and 5, reach 0 and 1.  host_lin_r{0,1} / host_reg5_r{0,1}: capi.host_map_register on the
                    same inputs (one core); the first round's counts are equal and the poses agree to 1e-5 m / 1e-5 rad (asserted).
                    surfels_download: Context.map_download_surfels of the same map — the pass a registration runs once per call.

The first two frames of a drive are left out; per drive the mean over frames, then median / p10 / p90 over the drives.  Prints one
JSON line.  The split of a round into surfels, terms, join and step comes from a kernel trace of --register-only
(profiles/map_register_time.md says how).
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

PARAMS = dict(max_dist=0.3, rho=0.1, min_count=5, flat=0.3)
MOMENTS = 1 << 20
ROUNDS = 5


def offset(T):
    w = np.array([0.010, -0.012, 0.015])
    th = np.linalg.norm(w)
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]) / th
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)
    D[:3, 3] = [0.03, -0.02, 0.04]
    return T @ D


def pose_distance(a, b):
    d = a["R"].T @ b["R"]
    return float(np.linalg.norm(a["t"] - b["t"])), float(np.arccos(np.clip((np.trace(d) - 1.0) / 2.0, -1.0, 1.0)))


def alone_legs(ctx, clouds, with_host=True, loops=1):
    """(iii): the last scan against the moments map of all of them"""
    pts, T = clouds[-1]
    T0 = offset(T)
    R, t = T0[:3, :3], np.array(T0[:3, 3])
    out = {}
    cids = [ctx.cloud_upload(p) for p, _ in clouds]
    own = ctx.map_create_mom(VOXEL, 1 << 18, 1 << 24, MOMENTS)
    try:
        for cid, (_, Tk) in zip(cids, clouds):
            ctx.map_insert_cloud(own, cid, Tk[:3, :3], Tk[:3, 3])
        dev = {}
        for _ in range(loops):
            for reach in (0, 1):
                ctx.map_register_cloud(own, cids[-1], R, t, ROUNDS, reach=reach, **PARAMS)  # (warm: the pooled scratch exists)
                t1 = time.perf_counter()
                lin = ctx.map_register_cloud(own, cids[-1], R, t, 0, reach=reach, **PARAMS)
                t2 = time.perf_counter()
                dev[reach] = ctx.map_register_cloud(own, cids[-1], R, t, ROUNDS, reach=reach, **PARAMS)
                t3 = time.perf_counter()
                assert np.array_equal(lin["counts"][0], dev[reach]["counts"][0])
                out["lin_r%d" % reach], out["reg5_r%d" % reach] = (t2 - t1) * 1e3, (t3 - t2) * 1e3
        t1 = time.perf_counter()
        ctx.map_download_surfels(own)
        out["surfels_download"] = (time.perf_counter() - t1) * 1e3
        out["shape"] = {"rows": ctx.map_size(own), "points": int(pts.shape[0]),
                        "counts_r0": [int(v) for v in dev[0]["counts"][0]], "counts_r1": [int(v) for v in dev[1]["counts"][0]],
                        "chi2_r1": [float(v) for v in dev[1]["chi2"]]}
        if with_host:
            h = capi.host_map_create_mom(VOXEL, 1 << 18, 1 << 24, MOMENTS)
            try:
                for p, Tk in clouds:
                    capi.host_map_insert(h, p, Tk[:3, :3], Tk[:3, 3])
                for reach in (0, 1):
                    t1 = time.perf_counter()
                    capi.host_map_register(h, pts, R, t, 0, reach=reach, **PARAMS)
                    t2 = time.perf_counter()
                    got = capi.host_map_register(h, pts, R, t, ROUNDS, reach=reach, **PARAMS)
                    t3 = time.perf_counter()
                    out["host_lin_r%d" % reach], out["host_reg5_r%d" % reach] = (t2 - t1) * 1e3, (t3 - t2) * 1e3
                    assert np.array_equal(got["counts"][0], dev[reach]["counts"][0]), "the host twin's first counts differ"
                    dt, da = pose_distance(got, dev[reach])
                    assert dt <= 1e-5 and da <= 1e-5, ("the host twin's pose differs", dt, da)
            finally:
                capi.host_map_destroy(h)
    finally:
        ctx.map_release(own)
        for cid in cids:
            ctx.cloud_release(cid)
    return out


def main():
    argv = sys.argv[1:]
    frame_only, register_only = "--frame-only" in argv, "--register-only" in argv
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

    if register_only:  # (for a kernel trace: the alone legs in a loop, nothing else on the device once the drive is done)
        kept = []
        plain_drive(keep=kept)
        legs = alone_legs(capi.Context.borrowed(), kept, with_host=False, loops=20)
        print(json.dumps({k: legs[k] for k in ("lin_r0", "lin_r1", "reg5_r0", "reg5_r1", "shape")}))
        return

    def child_drive(tree):
        env = dict(os.environ, MADICP_TREE=tree, PYTHONPATH=tree)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(frames), "1", "--frame-only"], env=env, cwd=tree,
                             capture_output=True, text=True, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])["off"][0]

    def mapped_drive(align):
        """(ii): the frame; the pose and the map it ends with, the last frame's alignment"""
        pl = pipeline()
        pl.setMapAccumulation(VOXEL, moments=MOMENTS)
        if align:
            pl.setMapAlignment(True, ROUNDS, 1, **PARAMS)
        ts = []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
        info = {"rows": int(pl.mapSize())}
        if align:
            pose, a = pl.mapFrameAlignment()
            T = np.asarray(pl.currentPose())
            info.update(last_frame_counts=[int(v) for v in a["counts"]], last_frame_chi2=[float(a["chi2_start"]), float(a["chi2"])],
                        last_frame_moved_m=float(np.linalg.norm(pose[:3, 3] - T[:3, 3])))
        return ms(ts), np.asarray(pl.currentPose()).tobytes() + pl.mapCloud().tobytes() + pl.mapMoments().tobytes(), info

    ctx = capi.Context.borrowed()
    plain_drive()  # (the first drive of a process pays for the pool's and the builder's first allocations)
    mapped_drive(True)
    if parent:
        child_drive(parent)
    alone = ("lin_r0", "lin_r1", "reg5_r0", "reg5_r1", "host_lin_r0", "host_lin_r1", "host_reg5_r0", "host_reg5_r1", "surfels_download")
    res = {k: [] for k in ("parent_off", "child_off", "align_off", "align_on") + alone}
    end, info, shape = {}, {}, {}
    for r in range(repeats):
        print("map_register_time: drive set %d of %d" % (r + 1, repeats), file=sys.stderr, flush=True)
        if parent:
            res["parent_off"].append(child_drive(parent))
            res["child_off"].append(child_drive(ROOT))
        for align, leg in ((False, "align_off"), (True, "align_on")):
            t, end[leg], info[leg] = mapped_drive(align)
            res[leg].append(t)
        assert end["align_off"] == end["align_on"], "the frame's alignment changed the pose or the map"
        kept = []
        plain_drive(keep=kept)
        legs = alone_legs(ctx, kept)
        for k in alone:
            res[k].append(legs[k])
        shape = legs["shape"]

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_and_maps_bit_equal": True, "voxel": VOXEL, "params": PARAMS, "rounds": ROUNDS}
    for k, v in res.items():
        if v:
            out[k] = stats(v)
    out["frame_map"] = info
    out["alone_shape"] = shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
