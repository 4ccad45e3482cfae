"""Pose evaluation timing: the HIP trajectory operator against the host.  Informational.

    python tools/pose_eval_bench.py [--frames 1591] [--repeats 5]

Workload: one synthetic drive of --frames frames (sequence 09 has 1 591) with synthetic
predictions (tests/pose_eval_case.py), track length 5.  In one run:

  operator  md2_pose_ate on device-resident operands, results left on the device
  numpy     the restated loop of tests/pose_eval_case.py (vectorised inverses, a Python
            loop of four-term products per snippet) on this host's CPU

GPU intervals are HIP events, the CPU loop time.perf_counter; one warm-up each, then the
median of --repeats.  Prints one JSON line.
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import pose_eval_case as pc  # noqa: E402
from monodepth2_amd.layers import transformation_from_parameters  # noqa: E402
from monodepth2_amd.pose_eval_ops import trajectory_ate, workspace_bytes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1591)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gt = pc.parse_text(pc.drive_text(args.frames, seed=9))
    aa, tr = pc.predictions(gt, seed=9)
    pred = transformation_from_parameters(torch.from_numpy(aa), torch.from_numpy(tr)).numpy()
    d_pred, d_gt = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    offsets = torch.tensor([0, args.frames], dtype=torch.int64).to(dev)
    ws = torch.empty(workspace_bytes(1, args.frames), dtype=torch.uint8, device=dev)

    trajectory_ate(d_pred, d_gt, offsets, workspace=ws)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ates, stats = trajectory_ate(d_pred, d_gt, offsets, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    t_op = statistics.median(times)

    cpu = []
    for _ in range(1 + min(args.repeats, 3)):
        t0 = time.perf_counter()
        want_a, want_s = pc.trajectory_ate_np(pred, gt)
        cpu.append((time.perf_counter() - t0) * 1e3)
    t_numpy = statistics.median(cpu[1:])

    got = np.concatenate([ates.cpu().numpy(), stats.cpu().numpy()[0]])
    want = np.concatenate([want_a, want_s])
    print(json.dumps({
        "frames": args.frames, "track_length": 5, "repeats": args.repeats, "synthetic_inputs": True,
        "hip_operator_ms": round(t_op, 4), "numpy_cpu_ms": round(t_numpy, 1),
        "mean": float(want_s[0]), "std": float(want_s[1]),
        "bit_equal_to_numpy": bool(np.array_equal(got.view(np.uint64), want.view(np.uint64))),
    }))


if __name__ == "__main__":
    main()
