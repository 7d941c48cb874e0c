"""Frame time of a stamped-deskew drive fed TWO SENSORS' RAW RECORDS against the same drive fed host-prepared arrays, one process.

  python tools/sources_frame_time.py [frames=16] [repeats=5]

The scans are the 120 k-point synthetic drive of tools/records_stamped_frame_time.py as a two-head rig would deliver it: two
buffers of about 60 k packed 22-byte records each (float32 x / y / z, an intensity, a ring, a uint32 nanosecond time counted from
each head's own message header), every head in its own sensor frame with a general sensor -> base extrinsic, about 3 % of the
records outside the range filter.  Three things are timed, interleaved drive by drive, `repeats` drives each:

  sources   pl.computeSourcesStamped(stamp, [Source, Source])   the two buffers as they are: filter, extrinsics, common clock,
                                                                 concatenation and the stamps on the device
  arrays    pl.compute(stamp, cloud, stamps)                     the same build fed what `prepare` made (made OUTSIDE the timed region)
  prepare   the host preparation the arrays caller needs first: per head the numpy unpack of the unaligned fields, the range filter
            in the sensor's frame, widening to float64, rotation and translation into the base frame, the times onto one clock;
            then concatenation, min / max and normalisation — per frame, on its own.  The transform is written in the evaluation
            order the library uses (three fused expressions instead of one matrix product) so that the two callers can be held to
            the same pose bits.

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
from mad_icp_amd.records import Source  # noqa: E402

B_MAX, B_MIN, RHO_KER, B_RATIO, K = 0.2, 0.1, 0.1, 0.02, 16
LO, HI = 0.7, 120.0
XYZIRT = np.dtype(dict(names=["x", "y", "z", "intensity", "ring", "t"], formats=["<f4", "<f4", "<f4", "<f4", "<u2", "<u4"],
                       offsets=[0, 4, 8, 12, 16, 18], itemsize=22))
SCALE = 1e-9
HEADER_NS = (0, 250000)  # the second head's message starts 0.25 ms after the first's


def extrinsic(seed):
    rng = np.random.default_rng([seed, 5])
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Q, rng.uniform(-1.0, 1.0, 3)
    return T


HEADS = (extrinsic(1), extrinsic(2))


def prepare(recs):
    """what a caller of compute(stamp, cloud, stamps) does on the host with the two drivers' buffers"""
    pts_all, tc_all, keep_all = [], [], []
    for rec, T, header in zip(recs, HEADS, HEADER_NS):
        x, y, z = rec["x"], rec["y"], rec["z"]
        with np.errstate(invalid="ignore", over="ignore"):
            nrm = np.sqrt(x * x + (y * y + z * z)).astype(np.float64)
            keep = ~((nrm < LO) | (nrm > HI) | np.isnan(x) | np.isnan(y) | np.isnan(z))
        o0, o1, o2 = x[keep].astype(np.float64), y[keep].astype(np.float64), z[keep].astype(np.float64)
        R, t = T[:3, :3], T[:3, 3]
        pts = np.empty((o0.shape[0], 3))
        for i in range(3):
            pts[:, i] = t[i] + (R[i, 0] * o0 + (R[i, 1] * o1 + R[i, 2] * o2))
        pts_all.append(pts)
        tc = rec["t"].astype(np.float64) * SCALE
        tc_all.append(tc if header == 0 else tc + header * SCALE)
        keep_all.append(keep)
    tc, keep = np.concatenate(tc_all), np.concatenate(keep_all)
    t0, t1 = tc.min() + 0.0, tc.max() + 0.0
    return np.concatenate(pts_all, axis=0), np.ascontiguousarray(((tc - t0) / (t1 - t0))[keep])


def sources_of(recs):
    return [Source(rec, LO, HI, sensor_to_base=T, time_scale=SCALE, time_offset=header * SCALE)
            for rec, T, header in zip(recs, HEADS, HEADER_NS)]


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
        # the head starts at +pi and turns clockwise over 0.1 s: the model the azimuth path assumes
        ns = np.round((np.pi - np.arctan2(xyz[:, 1], xyz[:, 0])) / (2 * np.pi) * 1e8).astype(np.int64)
        h = xyz.shape[0] // 2
        recs = []
        for sl, T, header in zip((slice(0, h), slice(h, None)), HEADS, HEADER_NS):
            sensor = ((xyz[sl].astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)  # the points as this head sees them
            rec = np.zeros(sensor.shape[0], XYZIRT)
            rec["x"], rec["y"], rec["z"] = sensor[:, 0], sensor[:, 1], sensor[:, 2]
            rec["intensity"] = rng.uniform(0, 255, sensor.shape[0])
            rec["ring"] = rng.integers(0, 64, sensor.shape[0])
            rec["t"] = np.maximum(ns[sl] - header, 0)
            recs.append(rec)
        drive.append(recs)
    prepared = [prepare(recs) for recs in drive]
    rig = [sources_of(recs) for recs in drive]
    threads = min(os.cpu_count() or 1, 16)

    def one_drive(kind):
        if kind == "prepare":
            ts = []
            for recs in drive:
                t1 = time.perf_counter()
                prepare(recs)
                ts.append(time.perf_counter() - t1)
            return float(np.mean(ts[2:])) * 1e3, 0.0, None
        pl = pm.Pipeline(10.0, True, B_MAX, RHO_KER, 0.8, B_MIN, B_RATIO, K, threads, False)
        ts, build = [], []
        for i in range(frames):
            t1 = time.perf_counter()
            if kind == "sources":
                pl.computeSourcesStamped(0.1 * i, rig[i])
            else:
                pl.compute(0.1 * i, prepared[i][0], prepared[i][1])
            ts.append(time.perf_counter() - t1)
            build.append(pl.lastBuildMs())
        return float(np.mean(ts[2:])) * 1e3, float(np.mean(build[2:])), np.asarray(pl.currentPose())

    kinds = ("sources", "arrays", "prepare")
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
    assert np.array_equal(end["sources"].view(np.uint64), end["arrays"].view(np.uint64)), "the two callers ended on different poses"
    out = {"frames": frames, "frames_timed_per_drive": frames - 2, "drives_per_caller": repeats, "sources": 2,
           "records_per_source": [int(r.shape[0]) for r in drive[0]], "points_per_scan": int(prepared[0][0].shape[0]),
           "point_step": XYZIRT.itemsize, "host_threads": threads, "end_poses_bit_equal": True}
    for kind in kinds:
        out[kind + "_leg"] = {"ms_per_frame_median": round(float(np.median(res[kind])), 4),
                              "ms_per_frame_p10": round(float(np.percentile(res[kind], 10)), 4),
                              "ms_per_frame_p90": round(float(np.percentile(res[kind], 90)), 4),
                              "ms_per_frame_drives": [round(x, 4) for x in res[kind]]}
        if kind != "prepare":
            out[kind + "_leg"]["front_end_ms_median"] = round(float(np.median(front[kind])), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
