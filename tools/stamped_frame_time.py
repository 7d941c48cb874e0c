"""Frame time of a deskewed drive: the azimuth caller against the stamped caller, same scans, one process.

  python tools/stamped_frame_time.py [frames=16] [repeats=5]

Both callers are unmodified-default Pipelines with deskew = True (the device front-end), fed the 120 k-point synthetic drive
bench.py's pipeline_end_to_end.default_deskew uses (same scene, path, seeds and 1e-7 m jitter):

  azimuth   pl.compute(stamp, cloud)            madicp_cloud_deskew: atan2 keys, radix sort, targets, prefix minimum, apply
  stamped   pl.compute(stamp, cloud, stamps)    madicp_cloud_deskew_stamped: one streaming kernel (+ n doubles over PCIe)

The stamps are what a spinning sensor's driver would deliver for these scans — s = (pi - azimuth) / (2 pi): the head starts at
+pi and turns clockwise, the model the azimuth path assumes — so the two callers compensate nearly the same way and register
nearly the same clouds.  compute() returns after the registration's result has been read back, so a host clock around it is a
synchronised time.  The two callers alternate, `repeats` drives each; the first two frames of a drive (no deskew yet, first
allocations) are left out; per drive the mean over frames, then median / min / max over the drives.  Prints one JSON line.
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


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    from mad_icp.src.pybind import pypeline as pm

    scene = synth.Scene(0)
    jitter = np.random.default_rng(0)
    drive = []
    for i in range(frames):
        sc = synth.render_scan(scene, synth.path_pose(1.0 * i), 100 + i)
        drive.append(np.ascontiguousarray(sc + jitter.normal(scale=1e-7, size=sc.shape)))
    stamps = [np.ascontiguousarray((np.pi - np.arctan2(sc[:, 1], sc[:, 0])) / (2 * np.pi)) for sc in drive]
    threads = min(os.cpu_count() or 1, 16)

    def one_drive(stamped):
        pl = pm.Pipeline(10.0, True, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, K, threads, False)
        ts, build = [], []
        for i, sc in enumerate(drive):
            t1 = time.perf_counter()
            if stamped:
                pl.compute(0.1 * i, sc, stamps[i])
            else:
                pl.compute(0.1 * i, sc)
            ts.append(time.perf_counter() - t1)
            build.append(pl.lastBuildMs())
        return float(np.mean(ts[2:])) * 1e3, float(np.mean(build[2:])), np.asarray(pl.currentPose())

    one_drive(False)  # (the first drive of a process pays for the pool's and the builder's first allocations)
    one_drive(True)
    res = {"azimuth": [], "stamped": []}
    front = {"azimuth": [], "stamped": []}
    end = {}
    for _ in range(repeats):
        for key, st in (("azimuth", False), ("stamped", True)):
            ms, b, pose = one_drive(st)
            res[key].append(ms)
            front[key].append(b)
            end[key] = pose
    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_caller": repeats,
           "points_per_scan": int(drive[0].shape[0]), "host_threads": threads}
    for key in res:
        out[key] = {"ms_per_frame_median": round(float(np.median(res[key])), 4), "ms_per_frame_min": round(min(res[key]), 4),
                    "ms_per_frame_max": round(max(res[key]), 4), "ms_per_frame_drives": [round(x, 4) for x in res[key]],
                    "front_end_ms_median": round(float(np.median(front[key])), 4)}
    out["end_pose_translation_difference_m"] = round(float(np.linalg.norm(end["azimuth"][:3, 3] - end["stamped"][:3, 3])), 6)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
