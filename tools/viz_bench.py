"""Disparity-picture timing: the HIP colour-map operator against the host.  Informational.

    python tools/viz_bench.py [--images 697] [--repeats 5] [--host-images 8] [--out profiles/viz_bench.json]

Workload: --images synthetic 192 x 640 disparity maps (the Eigen test split has 697) resized
to 375 x 1242, 95th percentile.  In one run:

  operator    md2_disp_colorize on device-resident operands, one call for the whole batch,
              results left on the device
  numpy       the restatement of tests/viz_case.py on this host's CPU
  matplotlib  the reference's path (torch CPU interpolate, np.percentile, Normalize,
              ScalarMappable) where matplotlib imports

The host paths run on the first --host-images maps, one at a time as the reference does, and
are reported per image and scaled to --images.  GPU intervals are HIP events, the host
time.perf_counter; one warm-up each, then the median of --repeats.  Prints one JSON line and
writes it to --out.
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

import viz_case as vc  # noqa: E402
from monodepth2_amd.viz_ops import colorize_disparity, workspace_bytes  # noqa: E402

IN_HW, OUT_HW = (192, 640), (375, 1242)


def host_median(fn, maps, repeats):
    """Median over `repeats` (after one warm-up) of the time for all of `maps`, per image, ms."""
    times = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        for m in maps:
            fn(m)
        times.append((time.perf_counter() - t0) * 1e3 / len(maps))
    return statistics.median(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=697)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "viz_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    base = np.stack([vc.sigmoid_map(IN_HW[0], IN_HW[1], 100 + i) for i in range(args.host_images)])
    d_base = torch.from_numpy(base).to(dev)
    gain = torch.linspace(0.5, 1.0, args.images, device=dev).view(-1, 1, 1)
    disp = (d_base[torch.arange(args.images, device=dev) % args.host_images] * gain).unsqueeze(1).contiguous()
    disp[:args.host_images, 0] = d_base
    ws = torch.empty(workspace_bytes(args.images, IN_HW, OUT_HW), dtype=torch.uint8, device=dev)

    colorize_disparity(disp, OUT_HW, workspace=ws)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rgb = colorize_disparity(disp, OUT_HW, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    t_op = statistics.median(times)

    lut = vc.load_lut()
    t_numpy = host_median(lambda m: vc.colorize_np(m[None], OUT_HW, 95, lut), base, args.repeats)
    want = np.concatenate([vc.colorize_np(m[None], OUT_HW, 95, lut)[0] for m in base])
    got = rgb[:args.host_images].cpu().numpy()

    t_mpl = None
    try:
        import matplotlib
        import matplotlib.cm
        import matplotlib.colors

        def reference_path(m):
            r = torch.nn.functional.interpolate(torch.from_numpy(m)[None, None], OUT_HW, mode="bilinear",
                                                align_corners=False).squeeze().numpy()
            norm = matplotlib.colors.Normalize(vmin=r.min(), vmax=np.percentile(r, 95))
            mapper = matplotlib.cm.ScalarMappable(norm=norm, cmap="magma")
            return (mapper.to_rgba(r)[:, :, :3] * 255).astype(np.uint8)

        t_mpl = host_median(reference_path, base, args.repeats)
    except ImportError:
        pass

    n = OUT_HW[0] * OUT_HW[1]
    result = {
        "images": args.images, "in_hw": list(IN_HW), "out_hw": list(OUT_HW), "percentile": 95,
        "repeats": args.repeats, "host_images": args.host_images, "synthetic_inputs": True,
        "hip_operator_ms": round(t_op, 3), "hip_operator_us_per_image": round(t_op * 1e3 / args.images, 2),
        "hip_operator_gpixel_per_s": round(args.images * n / t_op / 1e6, 2),
        "numpy_cpu_ms_per_image": round(t_numpy, 2), "numpy_cpu_ms_scaled": round(t_numpy * args.images, 0),
        "matplotlib_cpu_ms_per_image": None if t_mpl is None else round(t_mpl, 2),
        "matplotlib_cpu_ms_scaled": None if t_mpl is None else round(t_mpl * args.images, 0),
        "byte_equal_to_numpy": bool(np.array_equal(got, want)),
    }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
