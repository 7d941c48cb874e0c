"""Drive a SHARDED Pipeline (Pipeline::setShard through sharded.shard_pipeline): spawns N ranks, every
rank feeds its own Pipeline the same M synthetic full-size scans, and prints frames/s per transport (rank 0's clock; every
rank returns from a frame's registration together) with the unsharded Pipeline of one process beside it.

    python tools/pipeline_sharded_drive.py --ranks 8 --frames 60 --keyframes 16 --transports host,p2p

Ranks are dealt over the visible GPUs; with fewer GPUs than ranks several ranks SHARE a device (each on its own slice of the
CU mask, MADICP_CU_MASK=i/n, over gloo: RCCL refuses several ranks on one GPU, so `native` is then skipped) and the figure is
labelled "functional, ranks share one GPU": it says that the path works, not how it scales — nothing crosses xGMI there.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(a):
    return (10.0, False, 0.2, 0.1, a.p_th, 0.1, 0.02, a.keyframes, 16, False)


def _scans(a):
    from mad_icp_amd import synth

    scene = synth.Scene(a.scene)
    return [synth.render_scan(scene, synth.path_pose(a.step * i), 4000 + 97 * a.scene + i) for i in range(a.frames)]


def _drive(pipe, scans, warmup):
    t0 = None
    for i, s in enumerate(scans):
        if i == warmup:
            t0 = time.perf_counter()
        pipe.compute(0.1 * i, s)
    return (len(scans) - warmup) / (time.perf_counter() - t0)


def _worker(rank, world, n_gpus, port, path, a, transports, out):
    shared = n_gpus < world
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if shared:
        os.environ["MAD_ICP_DEVICE"] = str(rank % max(n_gpus, 1))
        per_gpu = (world + n_gpus - 1) // n_gpus
        os.environ["MADICP_CU_MASK"] = "%d/%d" % (rank // n_gpus, per_gpu)
    else:
        os.environ["MAD_ICP_DEVICE"] = str(rank)
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    from mad_icp.src.pybind import pypeline
    from mad_icp_amd import sharded

    if not shared:
        torch.cuda.set_device(rank)
    dist.init_process_group("gloo" if shared else "nccl", rank=rank, world_size=world)
    try:
        z = np.load(path)
        scans = [z["s%d" % i] for i in range(a.frames)]
        res = {}
        for t in transports:
            pipe = pypeline.Pipeline(*_args(a))
            ctx = sharded.shard_pipeline(pipe, transport=t, allow_coarse=shared)
            dist.barrier()
            res[t + "_fps"] = _drive(pipe, scans, a.warmup)
            res[t + "_pose"] = np.asarray(pipe.currentPose())
            res[t + "_local"] = pipe.numLocalKeyframes()
            del pipe
            sharded.unshard(ctx)
        np.savez(out % rank, **res)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--keyframes", type=int, default=16)
    ap.add_argument("--scene", type=int, default=0)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--p-th", dest="p_th", type=float, default=0.8)
    ap.add_argument("--transports", default="native,host,p2p")
    a = ap.parse_args()
    if not (1 <= a.ranks <= 8) or a.warmup >= a.frames:
        ap.error("1 <= ranks <= 8 (one node) and warmup < frames")

    import tempfile

    import torch
    import torch.multiprocessing as mp

    from mad_icp_amd import _build

    _build.build_all()
    from mad_icp.src.pybind import pypeline

    n_gpus = torch.cuda.device_count()
    if n_gpus < 1:
        sys.exit("no GPU: the Pipeline has no CPU path")
    shared = n_gpus < a.ranks
    transports = [t for t in a.transports.split(",") if t]
    if shared and "native" in transports:
        print("(native skipped: RCCL refuses several ranks on one GPU)")
        transports.remove("native")
    label = " [functional, ranks share one GPU]" if shared else ""
    scans = _scans(a)
    print("%d frames x %d points, %d keyframes, scene %d, %.1f m per frame, p_th %.2f; %d ranks on %d GPU(s)"
          % (a.frames, scans[0].shape[0], a.keyframes, a.scene, a.step, a.p_th, a.ranks, n_gpus))
    one = pypeline.Pipeline(*_args(a))
    fps1 = _drive(one, scans, a.warmup)
    pose1 = np.asarray(one.currentPose())
    del one
    print("  unsharded, one process: %8.1f frames/s" % fps1)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scans.npz")
        np.savez(path, **{"s%d" % i: s for i, s in enumerate(scans)})
        out = os.path.join(tmp, "rank%d.npz")
        port = 21000 + (os.getpid() * 7) % 4000
        mp.spawn(_worker, args=(a.ranks, n_gpus, port, path, a, transports, out), nprocs=a.ranks, join=True)
        R = [np.load(out % r) for r in range(a.ranks)]
    for t in transports:
        same = all(np.array_equal(R[0][t + "_pose"], r[t + "_pose"]) for r in R[1:])
        print("  sharded over %d ranks, %-6s: %8.1f frames/s%s; trees per rank at the end %s; last pose %s on every rank, %.2e m from "
              "the unsharded one" % (a.ranks, t, float(R[0][t + "_fps"]), label, [int(r[t + "_local"]) for r in R],
                                     "bit-equal" if same else "NOT EQUAL", float(np.linalg.norm(R[0][t + "_pose"][:3, 3] - pose1[:3, 3]))))


if __name__ == "__main__":
    main()
