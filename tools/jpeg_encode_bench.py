"""Device JPEG encoder timing: md2_jpeg_encode against Pillow, and packs with and without
transcoding.  Informational; no bar is set on these numbers.

    python tools/jpeg_encode_bench.py [--frames 64] [--height 375] [--width 1242] [--quality 92]
                                      [--sampling 4:2:0] [--repeats 5] [--sections encode pillow pack]
                                      [--tree-frames 640] [--out profiles/jpeg_encode_bench.json]

Workload: --frames `textured` frames (tests/jpeg_case.py) of 375 x 1242, already on the device.

  encode  md2_jpeg_encode on the device-resident frames, tables and output ranges (bound
          capacity), warm; HIP events around as many calls as fill a second, the median of
          --repeats such intervals per call.  The first stream is compared with Pillow's.
  pillow  Image.save(quality, subsampling) into memory of the same frames on 1 and on 16 host
          threads (time.perf_counter, best of 3)
  pack    pack.build_pack(png=True) with and without transcode on a synthetic tree of
          --tree-frames PNG files of that size (one drive, one camera), end to end, with both
          packs' sizes
  kernels two encode calls and nothing else: the process to run under
          `rocprofv3 --kernel-trace --stats` for the per-kernel times

Bytes per pass are counted from the shapes (reads of RGB counted once per component that
reads them; coefficients 128 bytes per block).  A run that finds no GPU fails.  Prints one
JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import jpeg_case as jc  # noqa: E402
from monodepth2_amd import jpeg_ops  # noqa: E402

DRIVE = "2011_09_26/2011_09_26_drive_0001_sync"


def staged_call(frames, quality, sampling, dev):
    """Everything md2_jpeg_encode needs on the device; returns a callable that runs one call."""
    n = len(frames)
    shapes = [f.shape[:2] for f in frames]
    offs = np.concatenate([[0], np.cumsum([f.size for f in frames])]).astype(np.int64)
    images, quant, out_bytes = jpeg_ops.describe_encode(shapes, [sampling] * n, [quality] * n, offs[:-1].tolist())
    tb = (jpeg_ops.encode_tables_bytes(n, len(quant)) + 15) // 16 * 16
    host = np.zeros(tb + int(offs[-1]), np.uint8)
    jpeg_ops.fill_encode_tables(host, images, n, quant)
    host[tb:] = np.concatenate([f.reshape(-1) for f in frames])
    staged = torch.from_numpy(host).to(dev)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)

    def call():
        return jpeg_ops.run_encode(staged, staged[tb:], images, n, len(quant), out, dev)
    return call, out, images


def bench_encode(frames, quality, sampling, dev, repeats):
    call, out, images = staged_call(frames, quality, sampling, dev)
    for _ in range(3):
        lengths, status = call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    calls = max(int(1.0 / max(time.perf_counter() - t0, 1e-4)) + 1, 5)
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            lengths, status = call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / calls)
    lens = lengths.cpu().numpy()
    first = out[images[0].out_offset:images[0].out_offset + int(lens[0])].cpu().numpy().tobytes()
    want = jpeg_ops.parse_jpeg(jc.encode(frames[0], {0: "4:4:4", 1: "4:2:2", 2: "4:2:0"}[sampling], quality)).data
    return {"calls_per_interval": calls, "ms_per_call": round(statistics.median(times), 4),
            "ms_per_call_min": round(min(times), 4), "ms_per_call_max": round(max(times), 4),
            "frames_per_s": round(len(frames) / (statistics.median(times) * 1e-3), 1),
            "stream_bytes": int(lens.sum()), "status_all_zero": bool(int(status.abs().sum()) == 0),
            "first_stream_equals_pillow": first == want}


def bench_pillow(frames, quality, sampling):
    def save(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=sampling)
        return buf.tell()
    out = {}
    for threads in (1, 16):
        best = None
        with ThreadPoolExecutor(threads) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                list(pool.map(save, frames))
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
        out[f"threads_{threads}_ms"] = round(best * 1e3, 2)
        out[f"threads_{threads}_frames_per_s"] = round(len(frames) / best, 1)
    return out


def traffic(frames, sampling):
    """Bytes each pass moves for the batch, from the shapes."""
    hs, vs = {0: (1, 1), 1: (2, 1), 2: (2, 2)}[sampling]
    rgb = blocks = 0
    for f in frames:
        h, w = f.shape[:2]
        blocks += -(-w // (8 * hs)) * -(-h // (8 * vs)) * (hs * vs + 2)
        rgb += h * w * 3
    return {"blocks": blocks, "dct_read_rgb": 3 * rgb, "dct_write_coef": 128 * blocks,
            "count_read_coef": 128 * blocks, "count_write_bits": 4 * blocks,
            "scan_read_bits": 4 * blocks, "scan_write_offsets": 8 * blocks,
            "emit_read_coef": 128 * blocks, "emit_read_offsets": 12 * blocks,
            "zero_and_emit_write": "2 x stream_bytes"}


def bench_pack(n, h, w, quality, sampling, dev):
    from monodepth2_amd.pack import build_pack
    root = tempfile.mkdtemp(prefix="md2_encbench_")
    try:
        folder = os.path.join(root, DRIVE, "image_02/data")
        os.makedirs(folder)

        def write(i):
            Image.fromarray(jc.textured(h, w, i)).save(os.path.join(folder, "%010d.png" % i), compress_level=1)
        with ThreadPoolExecutor(16) as pool:
            list(pool.map(write, range(n)))
        lines = ["{} {} l".format(DRIVE, i) for i in range(1, n - 1)]
        out = {"tree_frames": n, "png_bytes": sum(os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder))}
        for name, kw in (("raw", {}), ("transcoded", {"transcode": (quality, sampling)})):
            path = os.path.join(root, name + ".pack")
            build_pack(path, root, [lines[:8]], png=True, device=dev, threads=16, **kw)     # warm
            t0 = time.perf_counter()
            stats = build_pack(path, root, [lines], png=True, device=dev, threads=16, **kw)
            dt = time.perf_counter() - t0
            out[name] = {"seconds": round(dt, 3), "frames_per_s": round(stats["frames"] / dt, 1),
                         "pack_bytes": stats["pack_bytes"], "frames": stats["frames"],
                         "transcoded": stats["transcoded"]}
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--quality", type=int, default=92)
    ap.add_argument("--sampling", default="4:2:0")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree-frames", type=int, default=640)
    ap.add_argument("--sections", nargs="+", default=["encode", "pillow", "pack"],
                    choices=["encode", "pillow", "pack", "kernels"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_encode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_encode_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    sampling = jpeg_ops.sampling_class(args.sampling)
    frames = [jc.textured(args.height, args.width, 100 + i) for i in range(args.frames)]
    if "kernels" in args.sections:
        call, _, _ = staged_call(frames, args.quality, sampling, dev)
        call()
        call()
        torch.cuda.synchronize()
        return
    result = {"frames": args.frames, "height": args.height, "width": args.width, "quality": args.quality,
              "sampling": args.sampling, "repeats": args.repeats, "synthetic_inputs": True,
              "traffic_bytes": traffic(frames, sampling), "device": torch.cuda.get_device_name(0)}
    for section in ("encode", "pillow", "pack"):
        result[section] = "not measured"
    if "encode" in args.sections:
        result["encode"] = bench_encode(frames, args.quality, sampling, dev, args.repeats)
    if "pillow" in args.sections:
        result["pillow"] = bench_pillow(frames, args.quality, sampling)
    if "pack" in args.sections:
        result["pack"] = bench_pack(args.tree_frames, args.height, args.width, args.quality, sampling, dev)
    result["note"] = ("tools/jpeg_encode_bench.py on one MI355X, 16 host CPUs; encode: device-resident frames, HIP "
                      "events; pillow: the same frames saved into memory on this host; pack: build_pack end to end "
                      "on PNG files just written (page cache); informational")
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
