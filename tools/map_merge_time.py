"""What merging saved rows into the voxel map costs: the frame with nothing of it called against the parent commit's frame, one
restore of a drive's map, one merge of that batch into a map that already holds it, the host twin beside both, and what the
restore replaces — folding the drive's scans again.

  python tools/map_merge_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/map_merge_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)

The scans are the 120 k-point synthetic drive of tools/map_prune_time.py (22-byte XYZIRT records, 1 m per frame), fed to default
Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive, `repeats` drives each:

  (a) parent_off / child_off   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call, accumulation off — of
                    ANOTHER built tree of this project (--parent TREE: the parent commit's) and of THIS tree, each in a child
                    process per drive (this file with --frame-only, which touches nothing the parent lacks): child against child.
  For each kind of map — plain, ev (evidence (2, 1, 6)), mom (evidence and moments, max_count 2^20) — at voxel 0.2 m, the map of
  the whole drive built outside the clock by folding the registered scans at their poses, its columns downloaded:
  (b) restore_{kind}      one Context.map_merge_rows of all its rows into a fresh, EMPTY device map made with room for them (no
                    growth inside the clock): a host clock around the call — the staging copy, the upload, the kernels, the one
                    host synchronisation.
      present_{kind}      the same batch merged into the map that already holds every key: no row added.
      host_restore_{kind} / host_present_{kind}   the host twin (capi.HostMap.merge_rows), the same batches.
  (c) refold_{kind}       what a restore replaces: Context.map_insert_cloud of every scan of the drive (resident, uploaded outside
                    the clock) into a fresh map — the sum over the drive.
  The restored device map's columns are asserted byte-equal to the saved ones, and to the host twin's.

The first two frames of a drive are left out of (a); per drive one value per leg, then median / p10 / p90 over the drives.  Prints
one JSON line.
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

KINDS = {"plain": dict(), "ev": dict(evidence=(2, 1, 6)), "mom": dict(evidence=(2, 1, 6), max_count=1 << 20)}


def columns(m, spec):
    rows, keys = m.download_rows(with_keys=True)
    return dict(keys=keys, rows=rows, ev=m.download_evidence() if spec.get("evidence") else None,
                mom=m.download_moments() if spec.get("max_count") else None)


def same(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


def merge_legs(ctx, clouds):
    """(b) and (c) for every kind: the drive's scans (points, pose) are uploaded once, outside every clock"""
    out, shape = {}, {}
    cids = [ctx.cloud_upload(p) for p, _ in clouds]
    try:
        for kind, spec in KINDS.items():
            src = capi.DeviceMap.create(ctx, VOXEL, 1 << 18, 1 << 24, False, spec.get("evidence"), spec.get("max_count"))
            t0 = time.perf_counter()
            for cid, (_, T) in zip(cids, clouds):
                src.insert(cid, T[:3, :3], T[:3, 3])
            n = src.size()  # (every fold has ended in its own synchronisation)
            out["refold_" + kind] = (time.perf_counter() - t0) * 1e3
            saved = columns(src, spec)
            batch = (VOXEL, saved["keys"], saved["rows"], None, saved["ev"], saved["mom"])
            for side, make in (("", lambda: capi.DeviceMap.create(ctx, VOXEL, 1 << 18, 1 << 24, False, spec.get("evidence"), spec.get("max_count"))),
                               ("host_", lambda: capi.HostMap.create(VOXEL, 1 << 18, 1 << 24, False, spec.get("evidence"), spec.get("max_count")))):
                warm = make()  # (the first merge of a size pays for the staging block and the pooled batch block)
                warm.merge_rows(*batch)
                warm.close()
                dst = make()
                t1 = time.perf_counter()
                got = dst.merge_rows(*batch)
                t2 = time.perf_counter()
                assert got == (n, n) and same(columns(dst, spec), saved), "the restored map is not the saved one (%s%s)" % (side, kind)
                t3 = time.perf_counter()
                again = dst.merge_rows(*batch)
                t4 = time.perf_counter()
                assert again == (0, n)
                out[side + "restore_" + kind], out[side + "present_" + kind] = (t2 - t1) * 1e3, (t4 - t3) * 1e3
                dst.close()
            shape[kind] = {"rows": int(n), "batch_bytes": int(sum(v.nbytes for v in saved.values() if v is not None))}
            src.close()
    finally:
        for cid in cids:
            ctx.cloud_release(cid)
    out["shape"] = shape
    return out


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

    def plain_drive(keep=None):
        pl = pm.Pipeline(10.0, True, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, K, threads, False)
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

    ctx = capi.Context.borrowed()
    plain_drive()  # (the first drive of a process pays for the pool's and the builder's first allocations)
    if parent:
        child_drive(parent)
    res = {k: [] for k in ("parent_off", "child_off")}
    shape = {}
    for r in range(repeats):
        print("map_merge_time: drive set %d of %d" % (r + 1, repeats), file=sys.stderr, flush=True)
        if parent:
            res["parent_off"].append(child_drive(parent))
            res["child_off"].append(child_drive(ROOT))
        kept = []
        plain_drive(keep=kept)
        legs = merge_legs(ctx, kept)
        shape = legs.pop("shape")
        for k, v in legs.items():
            res.setdefault(k, []).append(v)

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "voxel": VOXEL, "restored_columns_equal_saved": True}
    for k, v in res.items():
        if v:
            out[k] = stats(v)
    out["shape"] = shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
