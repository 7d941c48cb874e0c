"""What the voxel map's moments cost: the frame with moments off against the parent commit's frame, the frame of a cleared and ranged
0.2 m map without and with moments, one fold alone on a plain map and on a moments map, and the surfels of the whole map computed on
the device against downloading the moments and applying the same rule in numpy.

  python tools/map_moments_time.py [frames=16] [repeats=5] [--parent TREE] [--variant DIR]
  python tools/map_moments_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)
  python tools/map_moments_time.py --fold-only CLOUDS.npz                   (with MADICP_NATIVE_DIR=DIR: that build's library)

The scans are the 120 k-point synthetic drive of tools/map_prune_time.py (22-byte XYZIRT records, 1 m per frame; nothing moves in
it), fed to default Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive,
`repeats` drives each:

  (i)   parent_off / child_off   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call, accumulation off — of
                    ANOTHER built tree of this project (--parent TREE: the parent commit's) and of THIS tree, each in a child
                    process per drive (this file with --frame-only, which touches nothing the parent lacks): child against child.
  (ii)  mom_off / mom_on   the frame of a Pipeline with setMapAccumulation(0.2), setMapClearing(True) and setMapRange(20), with
                    moments=None and with moments=MAX_COUNT.  Both legs must end on the same pose and the same map rows, bit for bit
                    (asserted).
  (iii) fold_off / fold_on   one Context.map_insert_cloud of the last scan into the 0.2 m map of the scans before it (most of its
                    voxels are there already), on a map rebuilt outside the clock; off: madicp_map_create, on: madicp_map_create_mom.
  (iv)  surfels / moments_on_host   Context.map_download_surfels of the whole map of all scans against Context.map_download_moments +
                    map_download_keys + the same rule in numpy (vectorised; numpy.linalg.eigh for the eigen-solve); centroids and
                    counts must agree bit for bit (asserted).
  (v)   fold_on_child / fold_variant_child   (--variant DIR: the native libraries of this tree built into DIR with other defines, as
                    mad_icp_amd/_build.py does under MADICP_NATIVE_DIR / MADICP_EXTRA_DEFINES — -DMADICP_MOMENTS_PLAIN: ten
                    atomics per point instead of ten per run of equal rows in a wavefront) leg (iii)'s moments fold on the same
                    clouds in a child process per drive set that loads this tree's library, and in one that loads DIR's: child
                    against child.  The ten words of every row after the fold must agree bit for bit (asserted by digest).

MAX_COUNT is large enough that no row freezes within the drive: every candidate point pays its ten atomics in every fold.  The
first two frames of a drive are left out; per drive the mean over frames, then median / p10 / p90 over the drives.  Prints one JSON
line.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.environ.get("MADICP_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mad_icp_amd import capi  # noqa: E402
from map_prune_time import B_MAX, B_MIN, B_RATIO, HI, LO, RANGE, RHO_KER, VOXEL, K, make_drive, ms, stats  # noqa: E402

MARGIN = 0.0
MAX_COUNT = 1 << 20


def numpy_surfels(mom, keys, voxel):
    """csrc/common/voxel_moments.h's map_surfel over all rows at once: (centroid f32, normal f32, eigenvalues f32, count u32)"""
    m = mom.astype(np.float64)
    n = m[:, 0:1]
    mean = m[:, 1:4] / n
    cell = np.stack([((keys >> np.uint64(21 * a)) & np.uint64(0x1fffff)).astype(np.int64) - (1 << 20) for a in range(3)], axis=1)
    centroid = ((cell.astype(np.float64) + (mean + 0.5) / 65536.0) * voxel).astype(np.float32)
    C = np.empty((m.shape[0], 3, 3))
    for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, a, b] = C[:, b, a] = m[:, 4 + j] / n[:, 0] - mean[:, a] * mean[:, b]
    w, V = np.linalg.eigh(C)
    zero_at = 2.0 ** -24 * w[:, 2] + 4.0 * 2.0 ** -52 * (m[:, [4, 7, 9]] / n).max(axis=1)  # the zero rule
    w = np.where(w > zero_at[:, None], w, 0.0)
    s = voxel / 65536.0
    normal = np.where(n >= 3, V[:, :, 0], 0.0).astype(np.float32)
    return centroid, normal, (w * (s * s)).astype(np.float32), mom[:, 0].astype(np.uint32)


def alone_legs(ctx, clouds, moments):
    """(iii) and (iv): one fold alone on a freshly built map; then, on a moments map, the two ways to the surfels"""
    rays, T = clouds[-1]
    out = {}
    cids = [ctx.cloud_upload(pts) for pts, _ in clouds]
    own = ctx.map_create(VOXEL, 1 << 18, 1 << 24) if moments is None else ctx.map_create_mom(VOXEL, 1 << 18, 1 << 24, moments)
    try:
        for cid, (_, Tk) in list(zip(cids, clouds))[:-1]:
            ctx.map_insert_cloud(own, cid, Tk[:3, :3], Tk[:3, 3])
        t1 = time.perf_counter()
        added, rows = ctx.map_insert_cloud(own, cids[-1], T[:3, :3], T[:3, 3])
        out["fold"] = (time.perf_counter() - t1) * 1e3
        out["fold_shape"] = {"rows": rows, "added": added, "points": int(rays.shape[0])}
        if moments is not None:
            t1 = time.perf_counter()
            got = ctx.map_download_surfels(own)
            t2 = time.perf_counter()
            mom = ctx.map_download_moments(own)
            want = numpy_surfels(mom, ctx.map_download_keys(own), VOXEL)
            t3 = time.perf_counter()
            assert got[0].tobytes() == want[0].tobytes() and got[3].tobytes() == want[3].tobytes(), "device and numpy surfels differ"
            out["surfels"], out["moments_on_host"] = (t2 - t1) * 1e3, (t3 - t2) * 1e3
            out["surfels_shape"] = {"rows": int(got[0].shape[0]), "rows_with_3_points": int(np.count_nonzero(got[3] >= 3))}
            out["digest"] = hashlib.sha256(mom.tobytes()).hexdigest()
    finally:
        ctx.map_release(own)
        for cid in cids:
            ctx.cloud_release(cid)
    return out


def fold_only(path):
    """what --variant runs in a child per build: the clouds of one drive from `path`, two warm-up folds, then the timed one"""
    with np.load(path) as z:
        clouds = [(z["pts%d" % k], z["T%d" % k]) for k in range(int(z["count"]))]
    ctx = capi.Context(0)
    try:
        alone_legs(ctx, clouds, MAX_COUNT)
        alone_legs(ctx, clouds, MAX_COUNT)
        legs = alone_legs(ctx, clouds, MAX_COUNT)
    finally:
        ctx.close()
    print(json.dumps({"fold": legs["fold"], "digest": legs["digest"]}))


def main():
    argv = sys.argv[1:]
    if "--fold-only" in argv:
        return fold_only(argv[argv.index("--fold-only") + 1])
    frame_only = "--frame-only" in argv
    parent = variant = None
    if "--variant" in argv:
        at = argv.index("--variant")
        variant = os.path.abspath(argv[at + 1])
        del argv[at:at + 2]
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

    def mapped_drive(moments):
        """(ii): the frame; the pose and the map it ends with"""
        pl = pipeline()
        if moments is None:
            pl.setMapAccumulation(VOXEL)
        else:
            pl.setMapAccumulation(VOXEL, moments=moments)
        pl.setMapClearing(True, MARGIN)
        pl.setMapRange(RANGE)
        ts = []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
        info = {"rows": int(pl.mapSize()), "removed": int(pl.mapRemoved())}
        if moments is not None:
            n = pl.mapMoments()[:, 0]
            info["points_taken"] = int(n.sum())
            info["largest_n"] = int(n.max())
        return ms(ts), np.asarray(pl.currentPose()).tobytes() + pl.mapCloud().tobytes(), info

    ctx = capi.Context.borrowed()

    def child_fold(clouds, native_dir):
        env = dict(os.environ)
        env.pop("MADICP_NATIVE_DIR", None)
        if native_dir:
            env["MADICP_NATIVE_DIR"] = native_dir
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "clouds.npz")
            arrays = {"count": np.array(len(clouds))}
            for k, (pts, T) in enumerate(clouds):
                arrays["pts%d" % k], arrays["T%d" % k] = pts, T
            np.savez(path, **arrays)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--fold-only", path], env=env, capture_output=True, text=True,
                                 check=True).stdout
        return json.loads(out.strip().splitlines()[-1])

    plain_drive()  # (the first drive of a process pays for the pool's and the builder's first allocations)
    mapped_drive(MAX_COUNT)
    if parent:
        child_drive(parent)
    res = {k: [] for k in ("parent_off", "child_off", "mom_off", "mom_on", "fold_off", "fold_on", "surfels", "moments_on_host", "fold_on_child",
                           "fold_variant_child")}
    end, info, shape = {}, {}, {}
    for r in range(repeats):
        print("map_moments_time: drive set %d of %d" % (r + 1, repeats), file=sys.stderr, flush=True)
        if parent:
            res["parent_off"].append(child_drive(parent))
            res["child_off"].append(child_drive(ROOT))
        for moments, leg in ((None, "mom_off"), (MAX_COUNT, "mom_on")):
            t, end[leg], info[leg] = mapped_drive(moments)
            res[leg].append(t)
        assert end["mom_off"] == end["mom_on"], "moments changed the pose or the map"
        kept = []
        plain_drive(keep=kept)
        for moments, tag in ((None, "_off"), (MAX_COUNT, "_on")):
            legs = alone_legs(ctx, kept, moments)
            res["fold" + tag].append(legs["fold"])
            shape["fold" + tag] = legs["fold_shape"]
            if moments is not None:
                res["surfels"].append(legs["surfels"])
                res["moments_on_host"].append(legs["moments_on_host"])
                shape["surfels"] = legs["surfels_shape"]
        if variant:
            plain, other = child_fold(kept, None), child_fold(kept, variant)
            assert plain["digest"] == other["digest"], "the variant build's moments differ"
            res["fold_on_child"].append(plain["fold"])
            res["fold_variant_child"].append(other["fold"])

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_and_maps_bit_equal": True, "voxel": VOXEL, "margin": MARGIN, "range": RANGE,
           "max_count": MAX_COUNT, "variant_moments_bit_equal": bool(variant)}
    for k, v in res.items():
        if v:
            out[k] = stats(v)
    out["frame_map"] = {k: info[k] for k in ("mom_off", "mom_on")}
    out["alone_shape"] = shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
