"""What asking the voxel map costs: the frame with the option off against the parent commit's frame, the frame of a 0.2 m map without
and with setMapOverlap, one Context.map_query alone — both reaches, the scoring form and all per-point columns — against the host
twin and against what a consumer does today (download the rows and keys, index the keys on the host, apply the same rule), and the
one-lane-per-point kernel against the cooperative variant.

  python tools/map_query_time.py [frames=16] [repeats=5] [--parent TREE] [--variant DIR]
  python tools/map_query_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)
  python tools/map_query_time.py --query-only CLOUDS.npz                   (with MADICP_NATIVE_DIR=DIR: that build's library)

The scans are the 120 k-point synthetic drive of tools/map_prune_time.py (22-byte XYZIRT records, 1 m per frame), fed to default
Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive, `repeats` drives each:

  (i)   parent_off / child_off   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call, accumulation off — of
                    ANOTHER built tree of this project (--parent TREE: the parent commit's) and of THIS tree, each in a child
                    process per drive (this file with --frame-only, which touches nothing the parent lacks): child against child.
  (ii)  overlap_off / overlap_on   the frame of a Pipeline with setMapAccumulation(0.2), without and with setMapOverlap(True, 1, 0.1).
                    Both legs must end on the same pose and the same map rows, bit for bit (asserted).
  (iii) query_r{0,1}_{score,full}   one Context.map_query of the last scan (resident, at its pose) against the 0.2 m map of the whole
                    drive, the map built outside the clock: reach 0 and 1, per_point=False (the three counts) and every column the
                    map has (row, d2, keys).  host_r{0,1}: capi.host_map_query on the same inputs (one core, a transient key index
                    per call), bit-equal (asserted).  consumer_r1: Context.map_download_rows (rows + keys) plus the same rule in
                    numpy through a sorted index of the keys — the vectorised form of a host-side dictionary — bit-equal (asserted).
  (iv)  lanes_child / coop_child   (--variant DIR: this tree's native libraries built into DIR with -DMADICP_QUERY_COOP, as
                    mad_icp_amd/_build.py does under MADICP_NATIVE_DIR / MADICP_EXTRA_DEFINES) the reach-1 queries of leg (iii), full
                    and (_score) scoring form, in a child process that loads this tree's library (fe::map_query_lanes: one lane
                    per point, 27 probes in a row) and in one that loads DIR's (fe::map_query_coop: 32 lanes per point): child
                    against child, the same bits (asserted by digest).

The first two frames of a drive are left out; per drive the mean over frames, then median / p10 / p90 over the drives.  Prints one
JSON line.
"""
import hashlib
import itertools
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
from map_prune_time import B_MAX, B_MIN, B_RATIO, HI, LO, RHO_KER, VOXEL, K, make_drive, ms, stats  # noqa: E402

MAX_DIST = 0.1
HALF = 1 << 20


def consumer_query(rows, keys, cloud, T, voxel, reach):
    """the rule of include/madicp_hip.h (madicp_map_query_cloud) on the host, from downloaded rows and keys: (row, d2)"""
    R, t = T[:3, :3], T[:3, 3]
    q = np.empty_like(cloud)
    for i in range(3):
        q[:, i] = t[i] + (R[i, 0] * cloud[:, 0] + (R[i, 1] * cloud[:, 1] + R[i, 2] * cloud[:, 2]))
    f = np.floor(q / voxel)
    cand = np.all((f >= -HALF) & (f < HALF), axis=1)
    cells = np.zeros(q.shape, np.int64)
    cells[cand] = f[cand].astype(np.int64)
    k64 = keys.astype(np.int64)
    order = np.argsort(k64, kind="stable")
    sk = k64[order]
    rows64 = rows.astype(np.float64)
    best_row, best_d2 = np.full(q.shape[0], 1 << 31, np.int64), np.full(q.shape[0], np.inf)
    for o in itertools.product(range(-reach, reach + 1), repeat=3):
        nb = cells + np.array(o, np.int64)
        idx = np.nonzero(cand & np.all((nb >= -HALF) & (nb < HALF), axis=1))[0]
        k = (nb[idx, 0] + HALF) | ((nb[idx, 1] + HALF) << 21) | ((nb[idx, 2] + HALF) << 42)
        at = np.minimum(np.searchsorted(sk, k), sk.size - 1)
        hit = sk[at] == k
        idx, j = idx[hit], order[at[hit]]
        d = q[idx] - rows64[j]
        d2 = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        first = (d2 < best_d2[idx]) | ((d2 == best_d2[idx]) & (j < best_row[idx]))
        best_d2[idx[first]], best_row[idx[first]] = d2[first], j[first]
    return np.where(best_row == 1 << 31, -1, best_row).astype(np.int32), best_d2


def digest(answer):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in answer[1:]) + repr(answer[0]).encode()).hexdigest()


def alone_legs(ctx, clouds, with_host=True):
    """(iii): the last scan against the map of all of them"""
    pts, T = clouds[-1]
    R, t = T[:3, :3], T[:3, 3]
    out = {}
    cids = [ctx.cloud_upload(p) for p, _ in clouds]
    own = ctx.map_create(VOXEL, 1 << 18, 1 << 24)
    try:
        for cid, (_, Tk) in zip(cids, clouds):
            ctx.map_insert_cloud(own, cid, Tk[:3, :3], Tk[:3, 3])
        full = {}
        for reach in (0, 1):
            ctx.map_query(own, cids[-1], R, t, reach, MAX_DIST, per_point=False)  # (warm: the pooled scratch exists)
            t1 = time.perf_counter()
            score = ctx.map_query(own, cids[-1], R, t, reach, MAX_DIST, per_point=False)
            t2 = time.perf_counter()
            full[reach] = ctx.map_query(own, cids[-1], R, t, reach, MAX_DIST, with_keys=True)
            t3 = time.perf_counter()
            full[reach] = ctx.map_query(own, cids[-1], R, t, reach, MAX_DIST, with_keys=True)
            t4 = time.perf_counter()
            assert score == full[reach][0]
            out["query_r%d_score" % reach], out["query_r%d_full" % reach] = (t2 - t1) * 1e3, (t4 - t3) * 1e3
        out["digest"] = digest(full[1])
        out["shape"] = {"rows": ctx.map_size(own), "points": int(pts.shape[0]), "counts_r0": list(full[0][0]), "counts_r1": list(full[1][0])}
        if with_host:
            t1 = time.perf_counter()
            rows, keys = ctx.map_download_rows(own)
            t2 = time.perf_counter()
            row, d2 = consumer_query(rows, keys, pts, T, VOXEL, 1)
            t3 = time.perf_counter()
            assert row.tobytes() == full[1][1].tobytes() and d2.tobytes() == full[1][2].tobytes(), "the consumer's answer differs"
            out["consumer_r1"], out["consumer_r1_download"] = (t3 - t1) * 1e3, (t2 - t1) * 1e3
            h = capi.host_map_create(VOXEL, 1 << 18, 1 << 24)
            try:
                for p, Tk in clouds:
                    capi.host_map_insert(h, p, Tk[:3, :3], Tk[:3, 3])
                for reach in (0, 1):
                    t1 = time.perf_counter()
                    got = capi.host_map_query(h, pts, R, t, reach, MAX_DIST, with_keys=True)
                    out["host_r%d" % reach] = (time.perf_counter() - t1) * 1e3
                    assert digest(got) == digest(full[reach]), "the host twin's answer differs"
            finally:
                capi.host_map_destroy(h)
    finally:
        ctx.map_release(own)
        for cid in cids:
            ctx.cloud_release(cid)
    return out


def query_only(path):
    """what --variant runs in a child per build: the clouds of one drive from `path`, a warm-up pass, then the timed one"""
    with np.load(path) as z:
        clouds = [(z["pts%d" % k], z["T%d" % k]) for k in range(int(z["count"]))]
    ctx = capi.Context(0)
    try:
        alone_legs(ctx, clouds, with_host=False)
        legs = alone_legs(ctx, clouds, with_host=False)
    finally:
        ctx.close()
    print(json.dumps({"full": legs["query_r1_full"], "score": legs["query_r1_score"], "digest": legs["digest"]}))


def main():
    argv = sys.argv[1:]
    if "--query-only" in argv:
        return query_only(argv[argv.index("--query-only") + 1])
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

    def mapped_drive(overlap):
        """(ii): the frame; the pose and the map it ends with, the last frame's counts"""
        pl = pipeline()
        pl.setMapAccumulation(VOXEL)
        if overlap:
            pl.setMapOverlap(True, 1, MAX_DIST)
        ts = []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
        return ms(ts), np.asarray(pl.currentPose()).tobytes() + pl.mapCloud().tobytes(), {"rows": int(pl.mapSize()),
                                                                                          "last_frame_overlap": list(pl.mapFrameOverlap())}

    ctx = capi.Context.borrowed()

    def child_query(clouds, native_dir):
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
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--query-only", path], env=env, capture_output=True, text=True,
                                 check=True).stdout
        return json.loads(out.strip().splitlines()[-1])

    plain_drive()  # (the first drive of a process pays for the pool's and the builder's first allocations)
    mapped_drive(True)
    if parent:
        child_drive(parent)
    alone = ("query_r0_score", "query_r0_full", "query_r1_score", "query_r1_full", "host_r0", "host_r1", "consumer_r1", "consumer_r1_download")
    res = {k: [] for k in ("parent_off", "child_off", "overlap_off", "overlap_on", "coop_child", "lanes_child", "coop_child_score",
                           "lanes_child_score") + alone}
    end, info, shape = {}, {}, {}
    for r in range(repeats):
        print("map_query_time: drive set %d of %d" % (r + 1, repeats), file=sys.stderr, flush=True)
        if parent:
            res["parent_off"].append(child_drive(parent))
            res["child_off"].append(child_drive(ROOT))
        for overlap, leg in ((False, "overlap_off"), (True, "overlap_on")):
            t, end[leg], info[leg] = mapped_drive(overlap)
            res[leg].append(t)
        assert end["overlap_off"] == end["overlap_on"], "the overlap query changed the pose or the map"
        kept = []
        plain_drive(keep=kept)
        legs = alone_legs(ctx, kept)
        for k in alone:
            res[k].append(legs[k])
        shape = legs["shape"]
        if variant:
            lanes, coop = child_query(kept, None), child_query(kept, variant)
            assert coop["digest"] == lanes["digest"] == legs["digest"], "the variant build's answers differ"
            res["coop_child"].append(coop["full"])
            res["lanes_child"].append(lanes["full"])
            res["coop_child_score"].append(coop["score"])
            res["lanes_child_score"].append(lanes["score"])

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_and_maps_bit_equal": True, "voxel": VOXEL, "max_dist": MAX_DIST,
           "variant_answers_bit_equal": bool(variant)}
    for k, v in res.items():
        if v:
            out[k] = stats(v)
    out["frame_map"] = info
    out["alone_shape"] = shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
