"""Depth-evaluation timing: the fused HIP operator against the two formulations it replaces.

    python tools/eval_bench.py [--images 697] [--repeats 5] [--numpy-images 697]

Workload: the Eigen split's size — 697 images, network maps 192 x 640, ground truth
375 x 1242 at ~5 % density (synthetic values; the work does not depend on them), mono
evaluation (Eigen crop, range mask, per-image median scaling).  In one run:

  hip      evaluate_depth.evaluate_disparities on device-resident disparities and host
           ground truth (as np.load gives it): upload + one md2_depth_eval call + one
           read-back; and the md2_depth_eval chain alone on device-resident operands
  numpy    the reference's per-image loop (evaluate_depth.py:181-214) in numpy on this
           host's CPU, the resize as vectorised half-pixel bilinear (no cv2 here)
  eager    the same loop as eager torch ops on the same GPU (F.interpolate, boolean
           indexing, torch.median: the compute_depth_losses style), one host sync per image
           where the masked shapes are needed

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
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monodepth2_amd.eval_ops import depth_metrics, eigen_crop  # noqa: E402
from monodepth2_amd.evaluate_depth import evaluate_disparities  # noqa: E402
from monodepth2_amd.options import default_options  # noqa: E402

H, W, GH, GW = 192, 640, 375, 1242
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0


def make_inputs(n, device, distinct=8):
    g = torch.Generator(device=device).manual_seed(0)
    sig = torch.rand(distinct, 1, H // 8, W // 8, generator=g, device=device)
    sig = F.interpolate(sig, (H, W), mode="bilinear", align_corners=False) * 0.6 + 0.01
    depth = 1.0 / (0.01 + 9.99 * F.interpolate(sig, (GH, GW), mode="bilinear", align_corners=False)[:, 0])
    gt = depth * 3.0 * torch.exp(0.25 * torch.randn(distinct, GH, GW, generator=g, device=device))
    gt = torch.where(torch.rand(distinct, GH, GW, generator=g, device=device) < 0.05, gt, torch.zeros_like(gt))
    idx = torch.arange(n, device=device) % distinct
    return sig[idx].contiguous(), gt[idx].contiguous()


def resize_np(a, gh, gw):
    h, w = a.shape
    ys = np.maximum((np.arange(gh, dtype=np.float32) + np.float32(0.5)) * np.float32(h / gh) - np.float32(0.5), 0)
    xs = np.maximum((np.arange(gw, dtype=np.float32) + np.float32(0.5)) * np.float32(w / gw) - np.float32(0.5), 0)
    y0, x0 = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = (ys - y0)[:, None].astype(np.float32), (xs - x0)[None, :].astype(np.float32)
    r0, r1 = a[y0], a[y1]
    top = r0[:, x0] * (1 - fx) + r0[:, x1] * fx
    bot = r1[:, x0] * (1 - fx) + r1[:, x1] * fx
    return top * (1 - fy) + bot * fy


def errors_np(gt, pred):
    thresh = np.maximum(gt / pred, pred / gt)
    return ((np.abs(gt - pred) / gt).mean(), (((gt - pred) ** 2) / gt).mean(), np.sqrt(((gt - pred) ** 2).mean()),
            np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean()), (thresh < 1.25).mean(), (thresh < 1.25 ** 2).mean(),
            (thresh < 1.25 ** 3).mean())


def numpy_loop(scaled, gts):
    """evaluate_depth.py:181-214, eigen split, median scaling."""
    errors = []
    for pred_disp, gt_depth in zip(scaled, gts):
        gh, gw = gt_depth.shape
        pred_depth = 1 / resize_np(pred_disp, gh, gw)
        mask = np.logical_and(gt_depth > MIN_DEPTH, gt_depth < MAX_DEPTH)
        y0, y1, x0, x1 = eigen_crop(gh, gw)
        crop_mask = np.zeros(mask.shape)
        crop_mask[y0:y1, x0:x1] = 1
        mask = np.logical_and(mask, crop_mask)
        pred_depth, gt_depth = pred_depth[mask], gt_depth[mask]
        pred_depth *= np.median(gt_depth) / np.median(pred_depth)
        pred_depth[pred_depth < MIN_DEPTH] = MIN_DEPTH
        pred_depth[pred_depth > MAX_DEPTH] = MAX_DEPTH
        errors.append(errors_np(gt_depth, pred_depth))
    return np.array(errors).mean(0)


def eager_loop(scaled, gt, crop):
    """The same per-image work as eager torch ops on the device."""
    y0, y1, x0, x1 = crop
    crop_mask = torch.zeros(gt.shape[1:], dtype=torch.bool, device=gt.device)
    crop_mask[y0:y1, x0:x1] = True
    total = torch.zeros(7, device=gt.device)
    for i in range(scaled.shape[0]):
        pred = 1 / F.interpolate(scaled[i:i + 1], (gt.shape[1], gt.shape[2]), mode="bilinear", align_corners=False)[0, 0]
        g = gt[i]
        mask = (g > MIN_DEPTH) & (g < MAX_DEPTH) & crop_mask
        g, pred = g[mask], pred[mask]
        pred = torch.clamp(pred * (torch.median(g) / torch.median(pred)), MIN_DEPTH, MAX_DEPTH)
        thresh = torch.max(g / pred, pred / g)
        total += torch.stack([(torch.abs(g - pred) / g).mean(), ((g - pred) ** 2 / g).mean(),
                              torch.sqrt(((g - pred) ** 2).mean()),
                              torch.sqrt(((torch.log(g) - torch.log(pred)) ** 2).mean()),
                              (thresh < 1.25).float().mean(), (thresh < 1.25 ** 2).float().mean(),
                              (thresh < 1.25 ** 3).float().mean()])
    return total / scaled.shape[0]


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
    ap.add_argument("--images", type=int, default=697)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-images", type=int, default=None, help="images of the CPU loop (default: all)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sig, gt = make_inputs(args.images, dev)
    opt = default_options(eval_mono=True)
    gt_host = list(gt.cpu().numpy())

    t_e2e, res = gpu_ms(lambda: evaluate_disparities(sig, gt_host, opt, device=dev), args.repeats)
    t_chain, out = gpu_ms(lambda: depth_metrics(sig, gt, min_depth=opt.min_depth, max_depth=opt.max_depth),
                          args.repeats)
    scaled = 1.0 / opt.max_depth + (1.0 / opt.min_depth - 1.0 / opt.max_depth) * sig
    t_eager, eager = gpu_ms(lambda: eager_loop(scaled, gt, eigen_crop(GH, GW)), args.repeats)

    n_np = args.numpy_images or args.images
    scaled_host = scaled[:n_np, 0].cpu().numpy()
    numpy_loop(scaled_host[:4], gt_host[:4])
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        ref = numpy_loop(scaled_host, gt_host[:n_np])
        times.append((time.perf_counter() - t0) * 1e3)
    t_numpy = statistics.median(times) * args.images / n_np

    hip_mean = out[:, :7].double().mean(0).cpu().numpy()
    print(json.dumps({
        "images": args.images, "repeats": args.repeats, "numpy_images": n_np,
        "hip_evaluate_disparities_ms": round(t_e2e, 3), "hip_kernel_chain_ms": round(t_chain, 3),
        "eager_torch_gpu_ms": round(t_eager, 3), "numpy_cpu_ms": round(t_numpy, 1),
        "mean_errors_hip": [round(float(v), 6) for v in hip_mean],
        "mean_errors_e2e": [round(float(v), 6) for v in res["mean_errors"]],
        "mean_errors_eager": [round(float(v), 6) for v in eager.cpu().numpy()],
        "mean_errors_numpy": [round(float(v), 6) for v in ref],
    }))


if __name__ == "__main__":
    main()
