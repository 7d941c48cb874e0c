"""What the voxel map's evidence column costs and what it buys: the frame with evidence off against the parent commit's frame, the
frame of a cleared and ranged map with evidence off against on, one fold and one clearing alone off against on, the rows a cleared
map of the static drive ends with under several (hit, miss, cap), and mapConfirmed against downloading everything and filtering.

  python tools/map_evidence_time.py [frames=16] [repeats=5] [--parent TREE]
  python tools/map_evidence_time.py [frames] [repeats] --frame-only          (with MADICP_TREE=TREE: that tree's package)

The scans are the 120 k-point synthetic drive of tools/map_prune_time.py (22-byte XYZIRT records, 1 m per frame; nothing moves in
it), fed to default Pipelines (deskew = True, device front-end) through computeRecordsStamped.  Timed, interleaved drive by drive,
`repeats` drives each:

  (i)   parent_off / child_off   the frame — pl.computeRecordsStamped(...) alone, a host clock around the call, accumulation off — of
                    ANOTHER built tree of this project (--parent TREE: the parent commit's) and of THIS tree, each in a child
                    process per drive (this file with --frame-only, which touches nothing the parent lacks): child against child.
  (ii)  ev_off / ev_on   the frame of a Pipeline with setMapAccumulation(0.2), setMapClearing(True) and setMapRange(20), with
                    evidence=None and with evidence=EV.  All legs must end on the same pose, bit for bit (asserted); the maps differ.
  (iii) fold / clear_rays, each _off and _on   one Context.map_insert_cloud of the last scan into the 0.2 m map of the scans before it
                    (most of its voxels are there already: the hits), and one Context.map_clear_rays by the rays of the last scan
                    on the map of all scans, each on a map rebuilt outside the clock; off: madicp_map_create, on: madicp_map_create_ev.
  (iv)  rows        the rows a map with clearing on and no range ends the drive with, for every (hit, miss, cap) of SETTINGS, beside
                    the plain map with clearing and the plain map without; with the histogram of the words.  Not timed.
  (v)   confirmed / filter_on_host   pl.mapConfirmed(2) against pl.mapCloud() + pl.mapEvidence() + numpy filtering, on the map the
                    ev_on leg ends with; the two must agree bit for bit (asserted).

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
EV = (1, 1, 8)
SETTINGS = [(1, 1, 1), (1, 1, 8), (4, 1, 16), (2, 1, 8)]
MIN_E = 2


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

    def mapped_drive(evidence, clearing=True, ranged=True, confirm=False):
        """(ii), (iv) and (v): the frame; what the map ends with; the two ways to the confirmed rows, each under its own clock"""
        pl = pipeline()
        if evidence is None:
            pl.setMapAccumulation(VOXEL)
        else:
            pl.setMapAccumulation(VOXEL, evidence=evidence)
        if clearing:
            pl.setMapClearing(True, MARGIN)
        if ranged:
            pl.setMapRange(RANGE)
        ts = []
        for i, rec in enumerate(drive):
            t1 = time.perf_counter()
            pl.computeRecordsStamped(0.1 * i, rec, LO, HI)
            ts.append(time.perf_counter() - t1)
        info = {"rows": int(pl.mapSize()), "removed": int(pl.mapRemoved())}
        if evidence is not None:
            info["words"] = np.bincount(pl.mapEvidence()).tolist()
        if confirm:
            t1 = time.perf_counter()
            got = pl.mapConfirmed(MIN_E)
            t2 = time.perf_counter()
            rows, ev = pl.mapCloud(), pl.mapEvidence()
            want = rows[ev >= MIN_E]
            t3 = time.perf_counter()
            assert got.tobytes() == want.tobytes(), "mapConfirmed and the host's filtering differ"
            info["confirmed"], info["filter_on_host"], info["confirmed_rows"] = (t2 - t1) * 1e3, (t3 - t2) * 1e3, int(got.shape[0])
        return ms(ts), np.asarray(pl.currentPose()), info

    ctx = capi.Context.borrowed()

    def make_map(evidence):
        return ctx.map_create(VOXEL, 1 << 18, 1 << 24) if evidence is None else ctx.map_create_ev(VOXEL, 1 << 18, 1 << 24, *evidence)

    def alone_legs(clouds, evidence):
        """(iii): one fold and one clearing alone, each on a freshly built map"""
        rays, T = clouds[-1]
        R, t = T[:3, :3], T[:3, 3]
        out = {}
        cids = [ctx.cloud_upload(pts) for pts, _ in clouds]
        try:
            for what in ("fold", "clear_rays"):
                own = make_map(evidence)
                try:
                    for cid, (_, Tk) in list(zip(cids, clouds))[:-1]:
                        ctx.map_insert_cloud(own, cid, Tk[:3, :3], Tk[:3, 3])
                    if what == "fold":
                        t1 = time.perf_counter()
                        added, rows = ctx.map_insert_cloud(own, cids[-1], R, t)
                        out[what] = (time.perf_counter() - t1) * 1e3
                        out[what + "_shape"] = {"rows": rows, "added": added, "points": int(rays.shape[0])}
                    else:
                        ctx.map_insert_cloud(own, cids[-1], R, t)
                        rows = ctx.map_size(own)
                        t1 = time.perf_counter()
                        removed, _, _ = ctx.map_clear_rays(own, cids[-1], R, t, (0.0, 0.0, 0.0), MARGIN, rows)
                        out[what] = (time.perf_counter() - t1) * 1e3
                        out[what + "_shape"] = {"rows": rows, "removed": removed, "rays": int(rays.shape[0])}
                finally:
                    ctx.map_release(own)
        finally:
            for cid in cids:
                ctx.cloud_release(cid)
        return out

    plain_drive()  # (the first drive of a process pays for the pool's and the builder's first allocations)
    mapped_drive(EV)
    if parent:
        child_drive(parent)
    res = {k: [] for k in ("parent_off", "child_off", "ev_off", "ev_on", "confirmed", "filter_on_host", "fold_off", "fold_on", "clear_rays_off",
                           "clear_rays_on")}
    end, info, shape = {}, {}, {}
    for r in range(repeats):
        print("map_evidence_time: drive set %d of %d" % (r + 1, repeats), file=sys.stderr, flush=True)
        if parent:
            res["parent_off"].append(child_drive(parent))
            res["child_off"].append(child_drive(ROOT))
        for evidence, leg in ((None, "ev_off"), (EV, "ev_on")):
            t, pose, info[leg] = mapped_drive(evidence, confirm=evidence is not None)
            res[leg].append(t)
            end[leg] = pose.tobytes()
        assert end["ev_off"] == end["ev_on"], "evidence changed the pose"
        res["confirmed"].append(info["ev_on"].pop("confirmed"))
        res["filter_on_host"].append(info["ev_on"].pop("filter_on_host"))
        kept = []
        plain_drive(keep=kept)
        for evidence, tag in ((None, "_off"), (EV, "_on")):
            legs = alone_legs(kept, evidence)
            for what in ("fold", "clear_rays"):
                res[what + tag].append(legs[what])
                shape[what + tag] = legs[what + "_shape"]

    rows = {"plain_no_clearing": mapped_drive(None, clearing=False, ranged=False)[2], "plain_clearing": mapped_drive(None, ranged=False)[2]}
    for s in SETTINGS:
        rows["%d_%d_%d" % s] = mapped_drive(s, ranged=False)[2]

    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_leg": repeats, "records_per_scan": int(drive[0].shape[0]),
           "host_threads": threads, "end_poses_bit_equal": True, "voxel": VOXEL, "margin": MARGIN, "range": RANGE, "evidence": list(EV),
           "min_evidence": MIN_E}
    for k, v in res.items():
        if v:
            out[k] = stats(v)
    out["frame_map"] = {k: info[k] for k in ("ev_off", "ev_on")}
    out["alone_shape"] = shape
    out["rows_at_the_end_clearing_no_range"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
