"""Point-cloud export timing: the HIP operator against the host.  Informational.

    python tools/points_bench.py [--batch 16] [--height 375] [--width 1242] [--repeats 5] [--calls 20]
                                 [--out profiles/points_bench.json]

Workload: one chunk of `monodepth2_amd.pointcloud` — 16 uniform random disparity maps of
375 x 1242 with KITTI's intrinsics, near 0.15 (about a third of the pixels dropped, so the
compaction has work to do), stride 1.  In one run:

  operator  md2_depth_points (count, scan, emit) on device-resident operands with the
            caller's workspace, results left on the device
  numpy     the restatement of tests/points_case.py on this host's CPU (one run of one map,
            scaled by the batch)

GPU intervals are HIP events around --calls calls after five warm-up calls, the median of
--repeats such intervals divided by --calls; the CPU time is time.perf_counter.  Traffic is
counted from the shapes: per kept pixel 4 bytes of map and 3 of colour read and 15 written;
a dropped pixel's 4 bytes are not counted.  The share of the HBM peak is that traffic over the
operator's interval (launch gaps included: three launches) against 8 TB/s.  A run that finds
no GPU fails.  Prints one JSON line and writes it to --out.
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

import points_case as pc  # noqa: E402
from monodepth2_amd.points_ops import depth_to_points, workspace_bytes  # noqa: E402

HBM_PEAK = 8.0e12       # bytes / s, the MI355X's specified HBM3E peak
BYTES_PER_KEPT = 4 + 3 + 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "points_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/points_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    B, H, W = args.batch, args.height, args.width
    disp = np.random.RandomState(0).uniform(0.0, 1.0, (B, H, W)).astype(np.float32)
    rgb = pc.colours(B, H, W, 0)
    _, inv_K = pc.intrinsics(H, W, B)
    kw = dict(near=0.15)
    d_disp, d_rgb, d_k = (torch.from_numpy(a).to(dev) for a in (disp, rgb, inv_K))
    ws = torch.empty(workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)

    for _ in range(5):
        vertices, offsets = depth_to_points(d_disp, d_rgb, d_k, workspace=ws, **kw)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            vertices, offsets = depth_to_points(d_disp, d_rgb, d_k, workspace=ws, **kw)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / args.calls)
    t_op = statistics.median(times)
    kept = int(offsets[-1])

    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        rec, want_offsets, _, _ = pc.points_np(disp[:1], rgb[:1], inv_K[:1], **kw)
        cpu.append((time.perf_counter() - t0) * 1e3 * B)
    t_numpy = statistics.median(cpu[1:])
    n0 = int(want_offsets[-1])
    first = vertices[:15 * n0].cpu().numpy()

    traffic = BYTES_PER_KEPT * kept
    result = {
        "batch": B, "height": H, "width": W, "stride": 1, "near": kw["near"], "far": 80.0,
        "repeats": args.repeats, "calls_per_interval": args.calls, "synthetic_inputs": True,
        "pixels": B * H * W, "kept": kept,
        "hip_operator_ms": round(t_op, 4), "hip_operator_ms_min": round(min(times), 4),
        "hip_operator_ms_max": round(max(times), 4),
        "numpy_cpu_ms": round(t_numpy, 1),
        "bytes_per_kept_pixel": BYTES_PER_KEPT, "traffic_bytes": traffic,
        "traffic_tb_per_s": round(traffic / (t_op * 1e-3) / 1e12, 3),
        "share_of_hbm_peak_8tb": round(traffic / (t_op * 1e-3) / HBM_PEAK, 3),
        "first_image_byte_equal_to_numpy": bool(int(offsets[1]) == n0 and np.array_equal(first, rec.view(np.uint8))),
        "device": torch.cuda.get_device_name(0),
        "note": "tools/points_bench.py on one MI355X; the interval holds the operator's three launches and their "
                "gaps; numpy: the restatement of tests/points_case.py on the same machine's host CPU, one map "
                "timed and scaled by the batch; informational",
    }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
