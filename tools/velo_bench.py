"""Velodyne ground-truth export timing: the HIP projection operator against the host.

    python tools/velo_bench.py [--frames 697] [--points 120000] [--batch 64] [--repeats 5]
                               [--numpy-frames 64]

Workload: the Eigen split's size — 697 frames of 375 x 1242 with --points points each
(synthetic scans: a LiDAR-like fan in front of a KITTI-like camera, a tenth of the points
behind the sensor; 8 distinct scans repeated), the points' own forward distance as the
depth (what export_gt_depth.py asks for).  In one run:

  operator  md2_velo_project on device-resident points, offsets and matrices, --batch
            frames per call (the 16-byte-per-pixel workspace bounds the batch), maps left
            on the device
  e2e       kitti_utils.depth_maps_from_arrays from host arrays (what generate_depth_maps
            does after reading the files): concatenate, upload, project; maps on the device
  numpy     a vectorised numpy restatement of the reference's generate_depth_map (stable
            sort + reduceat instead of its Python loop over duplicates) on this host's
            CPU, --numpy-frames frames scaled to --frames

GPU intervals are HIP events (e2e includes the host work between them), the CPU loop
time.perf_counter; one warm-up each, then the median of --repeats.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monodepth2_amd.kitti_utils import depth_maps_from_arrays  # noqa: E402
from monodepth2_amd.velo_ops import project_velodyne, workspace_bytes  # noqa: E402

H, W = 375, 1242


def kitti_like_matrix():
    K = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
    M = np.eye(4)
    M[:3, :3] = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04], [1.480249e-02, 7.280733e-04, -9.998902e-01],
                          [9.998621e-01, 7.523790e-03, 1.480755e-02]])
    M[:3, 3] = [-4.069766e-03, -7.631618e-02, -2.717806e-01]
    return K @ M


def make_scan(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(2.0, 80.0, n)
    y = x * np.tan(rng.uniform(-0.75, 0.75, n))
    z = x * np.tan(rng.uniform(-0.42, 0.04, n))
    x[rng.uniform(size=n) < 0.1] *= -1
    return np.stack([x, y, z, rng.uniform(size=n)], 1).astype(np.float32)


def numpy_map(pts, P, vel_depth=True):
    """kitti_utils.py:46-98 vectorised (tests/velo_case.py holds the checked twin)."""
    pts = pts[pts[:, 0] >= 0]
    xyz = pts[:, :3].astype(np.float64)
    q = np.stack([((P[r, 0] * xyz[:, 0] + P[r, 1] * xyz[:, 1]) + P[r, 2] * xyz[:, 2]) + P[r, 3] for r in range(3)], 1)
    u, v = np.round(q[:, 0] / q[:, 2]) - 1, np.round(q[:, 1] / q[:, 2]) - 1
    ok = (u >= 0) & (v >= 0) & (u < W) & (v < H)
    u, v, d = u[ok].astype(np.int64), v[ok].astype(np.int64), (xyz[:, 0] if vel_depth else q[:, 2])[ok]
    depth = np.zeros(H * W)
    pix = v * W + u
    depth[pix] = d
    key = v * (W - 1) + u - 1
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    dup = np.diff(np.r_[start, len(ks)]) > 1
    depth[pix[order[start]][dup]] = np.minimum.reduceat(d[order], start)[dup]
    depth[depth < 0] = 0
    return depth.reshape(H, W).astype(np.float32)


def gpu_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=697)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-frames", type=int, default=64, help="frames of the CPU loop, scaled to --frames")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    distinct = [make_scan(args.points, s) for s in range(8)]
    scans = [distinct[i % 8] for i in range(args.frames)]
    P1 = kitti_like_matrix()
    batches = [(i, min(i + args.batch, args.frames)) for i in range(0, args.frames, args.batch)]

    # resident operands, one set per batch
    resident = []
    for a, b in batches:
        counts = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans[a:b]])]).astype(np.int64)
        resident.append((torch.from_numpy(np.concatenate(scans[a:b])).to(dev), torch.from_numpy(counts).to(dev),
                         torch.from_numpy(np.repeat(P1[None], b - a, 0)).to(dev)))
    ws = torch.empty(workspace_bytes(min(args.batch, args.frames), H, W, 1), dtype=torch.uint8, device=dev)

    def operator():
        out = None
        for pts, off, P in resident:
            out = project_velodyne(pts, off, P, H, W, vel_depth=True, workspace=ws)
        return out

    def e2e():
        out = None
        for a, b in batches:
            out = depth_maps_from_arrays(scans[a:b], np.repeat(P1[None], b - a, 0), H, W, vel_depth=True, device=dev)
        return out

    t_op, last = gpu_ms(operator, args.repeats)
    t_e2e, last_e2e = gpu_ms(e2e, args.repeats)

    n_np = min(args.numpy_frames, args.frames)
    numpy_map(scans[0], P1)
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        maps = [numpy_map(s, P1) for s in scans[:n_np]]
        times.append((time.perf_counter() - t0) * 1e3)
    t_numpy = statistics.median(times) * args.frames / n_np

    a, b = batches[-1]
    want = np.stack([numpy_map(s, P1) for s in scans[a:b][:4]])
    got, got_e2e = last[:4].cpu().numpy(), last_e2e[:4].cpu().numpy()
    print(json.dumps({
        "frames": args.frames, "points_per_frame": args.points, "batch": args.batch, "repeats": args.repeats,
        "numpy_frames": n_np, "synthetic_inputs": True,
        "hip_operator_ms": round(t_op, 3), "hip_operator_ms_per_frame": round(t_op / args.frames, 5),
        "hip_end_to_end_ms": round(t_e2e, 3), "hip_end_to_end_ms_per_frame": round(t_e2e / args.frames, 4),
        "numpy_cpu_ms": round(t_numpy, 1), "numpy_cpu_ms_per_frame": round(t_numpy / args.frames, 3),
        "occupied_pixels_per_frame": int(np.count_nonzero(want[0])),
        "bit_equal_to_numpy": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32))
                                   and np.array_equal(got_e2e.view(np.uint32), want.view(np.uint32))),
    }))


if __name__ == "__main__":
    main()
