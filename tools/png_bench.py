"""Device PNG decoder timing: md2_png_run against Pillow, transcoded packs and loader epochs
with and without it.  Informational; no bar is set on these numbers.

    python tools/png_bench.py [--frames 36 256] [--height 375] [--width 1242] [--repeats 5]
                              [--sections kernel pillow pack loader] [--tree-frames 640]
                              [--batch 12] [--threads 16] [--out profiles/png_decode.json]
    python tools/png_bench.py --sections indexed [--segment-bytes 16384] --repeats 3
                              --out profiles/png_indexed.json

Workload: `texture` frames (tools/loader_bench.py) of 375 x 1242 saved by Pillow with its
defaults (eight distinct frames, rolled sideways to make the others).

  kernel  md2_png_run on --frames streams already on the device, warm; HIP events around as
          many calls as fill a second (at least 3), the median of --repeats such intervals per
          call.  Every status word must be 0 and the first frame is compared with Pillow's.
  pillow  Image.open(...).convert("RGB") of the same files from memory on 1 and on 16 host
          threads (time.perf_counter, best of 3)
  pack    pack.build_pack(png=True, transcode=(92, 4:2:0)) with and without device_png on a tree
          of --tree-frames PNG files (one drive, one camera), end to end, alternated
  loader  an epoch of BatchLoader over that kind of tree read as .png, with and without
          device_png, at --batch and --threads, alternated epoch by epoch
  kernels two decode calls of the first --frames count and nothing else: the process to run under
          `rocprofv3 --kernel-trace --stats` for the per-kernel split
  indexed (not in the default list) md2_png_run_indexed against md2_png_run on
          the same --frames streams on the device, interval by interval in turn; the time of
          md2_png_index; a loader epoch from a KIND_PNG pack, from a KIND_RAW pack of the same
          tree and from the tree through PIL, epoch by epoch in turn; the bytes of both packs
  kernels_indexed  two md2_png_run_indexed calls of the first --frames count and nothing else

A run that finds no GPU fails.  Prints one JSON line and writes it to --out.
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from loader_bench import FRAME_IDS, H, S, W, epoch_time, texture  # noqa: E402
from monodepth2_amd import png_ops  # noqa: E402

DRIVE = "2011_09_26/2011_09_26_drive_0001_sync"


def frames_of(n, h, w):
    rng = np.random.default_rng(1)
    base = [texture(rng, h, w) for _ in range(min(n, 8))]
    return [np.roll(base[i % len(base)], 3 * (i // len(base)), axis=1) for i in range(n)]


def png_of(frame, **kw):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "PNG", **kw)
    return buf.getvalue()


def staged_call(files, dev):
    """Everything md2_png_run needs on the device; returns a callable that runs one call."""
    streams = [png_ops.parse_png(f) for f in files]
    if any(s is None for s in streams):
        raise SystemExit("parse_png refused a file Pillow wrote with its defaults")
    offsets, pos = [], 0
    for s in streams:
        offsets.append(pos)
        pos += (s.height * s.width * 3 + 255) // 256 * 256
    images, base, total = png_ops.describe_png_batch(streams, offsets)
    host = np.zeros(total, np.uint8)
    png_ops.fill_png_staging(host, streams, images, base)
    staged = torch.from_numpy(host).to(dev)
    out = torch.empty(pos, dtype=torch.uint8, device=dev)

    def call():
        return png_ops.run_png_staged(staged, images, len(streams), base, total, out, dev)
    return call, out, streams, offsets


def bench_kernel(files, first_frame, dev, repeats):
    call, out, streams, offsets = staged_call(files, dev)
    for _ in range(2):
        status = call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    calls = max(int(1.0 / max(time.perf_counter() - t0, 1e-4)) + 1, 3)
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            status = call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / calls)
    s = streams[0]
    got = out[offsets[0]:offsets[0] + s.height * s.width * 3].cpu().numpy().reshape(s.height, s.width, 3)
    med = statistics.median(times)
    return {"frames": len(files), "calls_per_interval": calls, "ms_per_call": round(med, 3),
            "ms_per_call_min": round(min(times), 3), "ms_per_call_max": round(max(times), 3),
            "frames_per_s": round(len(files) / (med * 1e-3), 1),
            "stream_bytes": sum(len(x.data) for x in streams),
            "raw_bytes": sum(x.height * (1 + 3 * x.width) for x in streams),
            "status_all_zero": bool(int(status.abs().sum()) == 0),
            "first_frame_equals_pillow": bool(np.array_equal(got, first_frame))}


def staged_call_indexed(files, dev, segment_bytes):
    """staged_call for md2_png_run_indexed; also returns the seconds md2_png_index took."""
    streams = [png_ops.parse_png(f) for f in files]
    png_ops.index_png_batch(streams[:2], segment_bytes, dev)      # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    indexes = png_ops.index_png_batch(streams, segment_bytes, dev)
    index_s = time.perf_counter() - t0
    offsets, pos = [], 0
    for s in streams:
        offsets.append(pos)
        pos += (s.height * s.width * 3 + 255) // 256 * 256
    images, index_offsets, base, total = png_ops.describe_png_batch_indexed(streams, indexes, offsets, segment_bytes)
    host = np.zeros(total, np.uint8)
    png_ops.fill_png_staging_indexed(host, streams, indexes, images, index_offsets, base)
    staged = torch.from_numpy(host).to(dev)
    out = torch.empty(pos, dtype=torch.uint8, device=dev)

    def call():
        return png_ops.run_png_staged_indexed(staged, images, index_offsets, len(streams), base, total, segment_bytes,
                                              out, dev)
    return call, out, streams, offsets, index_s, sum(len(ix) for ix in indexes)


def bench_indexed(files, first_frame, dev, repeats, segment_bytes):
    """md2_png_run and md2_png_run_indexed on the same streams, an interval of each in turn."""
    serial, out_s, streams, offsets = staged_call(files, dev)
    indexed, out_i, _, _, index_s, index_bytes = staged_call_indexed(files, dev, segment_bytes)
    times = {"serial": [], "indexed": []}
    status = {}
    for name, call in (("serial", serial), ("indexed", indexed)):
        status[name] = call()
        torch.cuda.synchronize()
    calls = {"serial": 3, "indexed": 10}
    for _ in range(repeats):
        for name, call in (("serial", serial), ("indexed", indexed)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls[name]):
                status[name] = call()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / calls[name])
    s = streams[0]
    got = out_i[offsets[0]:offsets[0] + s.height * s.width * 3].cpu().numpy().reshape(s.height, s.width, 3)
    res = {"frames": len(files), "index_seconds": round(index_s, 3), "index_bytes": index_bytes,
           "stream_bytes": sum(len(x.data) for x in streams),
           "same_bytes_as_serial": bool(torch.equal(out_s, out_i)),
           "first_frame_equals_pillow": bool(np.array_equal(got, first_frame))}
    for name in times:
        med = statistics.median(times[name])
        res[name] = {"ms_per_call": round(med, 3), "ms_per_call_all": [round(x, 3) for x in times[name]],
                     "frames_per_s": round(len(files) / (med * 1e-3), 1),
                     "status_all_zero": bool(int(status[name].abs().sum()) == 0)}
    res["speedup"] = round(res["serial"]["ms_per_call"] / res["indexed"]["ms_per_call"], 2)
    return res


def bench_loader_packs(root, lines, batch, threads, repeats, dev, segment_bytes):
    """A loader epoch from a KIND_PNG pack, from a KIND_RAW pack of the same tree and from the
    tree through PIL, epoch by epoch in turn; the packs' bytes and build times."""
    from monodepth2_amd.datasets import KITTIRAWDataset
    from monodepth2_amd.loader import BatchLoader
    from monodepth2_amd.pack import FramePack, build_pack
    out = {"batch": batch, "threads": threads, "segment_bytes": segment_bytes}
    packs = {}
    for name, kw in (("png_pack", dict(png_records=True, segment_bytes=segment_bytes)), ("raw_pack", {})):
        path = os.path.join(root, name + ".pack")
        t0 = time.perf_counter()
        stats = build_pack(path, root, [lines], png=True, device=dev, threads=threads, **kw)
        out[name] = {"build_seconds": round(time.perf_counter() - t0, 3), "pack_bytes": stats["pack_bytes"],
                     "png_records": stats["png"], "raw_records": stats["raw"], "file_bytes": stats["file_bytes"]}
        packs[name] = FramePack(path)
    ds = KITTIRAWDataset(root, lines, H, W, FRAME_IDS, S, is_train=True, img_ext=".png")
    loaders = {"pil": BatchLoader(ds, batch, shuffle=True, seed=0, num_workers=threads)}
    for name, fp in packs.items():
        loaders[name] = BatchLoader(ds, batch, shuffle=True, seed=0, num_workers=threads, pack=fp)
    times = {name: [] for name in loaders}
    n = 0
    for rep in range(repeats + 1):
        for name, ld in loaders.items():
            ld.set_epoch(rep)
            t, n = epoch_time(ld)
            if rep:
                times[name].append(t)
    out["batches"] = n
    for name, ld in loaders.items():
        t = statistics.median(times[name])
        out.setdefault(name, {}).update({"epoch_s": round(t, 3), "epoch_s_all": [round(x, 3) for x in times[name]],
                                         "frames_per_s": round(n * batch * len(FRAME_IDS) / t, 1)})
        ld.close()
    for fp in packs.values():
        fp.close()
    return out


def bench_pillow(files):
    def load(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).shape[0]
    out = {"frames": len(files)}
    for threads in (1, 16):
        best = None
        with ThreadPoolExecutor(threads) as pool:
            for _ in range(3):
                t0 = time.perf_counter()
                list(pool.map(load, files))
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
        out[f"threads_{threads}_ms"] = round(best * 1e3, 2)
        out[f"threads_{threads}_frames_per_s"] = round(len(files) / best, 1)
    return out


def write_tree(root, n, h, w):
    folder = os.path.join(root, DRIVE, "image_02/data")
    os.makedirs(folder)
    frames = frames_of(n, h, w)

    def write(i):
        Image.fromarray(frames[i]).save(os.path.join(folder, "%010d.png" % i))
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(write, range(n)))
    size = sum(os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder))
    return ["{} {} l".format(DRIVE, i) for i in range(1, n - 1)], size


def bench_pack(root, lines, dev, repeats, threads):
    from monodepth2_amd.pack import build_pack
    times = {"pil": [], "device_png": []}
    stats = {}
    for rep in range(repeats + 1):
        for name, flag in (("pil", False), ("device_png", True)):
            path = os.path.join(root, name + ".pack")
            t0 = time.perf_counter()
            stats[name] = build_pack(path, root, [lines if rep else lines[:8]], png=True, device=dev, threads=threads,
                                     transcode=(92, "4:2:0"), device_png=flag)
            if rep:
                times[name].append(time.perf_counter() - t0)
    out = {}
    for name in times:
        t = statistics.median(times[name])
        out[name] = {"seconds": round(t, 3), "seconds_all": [round(x, 3) for x in times[name]],
                     "frames": stats[name]["frames"], "frames_per_s": round(stats[name]["frames"] / t, 1),
                     "pack_bytes": stats[name]["pack_bytes"]}
    out["same_pack_bytes"] = out["pil"]["pack_bytes"] == out["device_png"]["pack_bytes"]
    return out


def bench_loader(root, lines, batch, threads, repeats):
    from monodepth2_amd.datasets import KITTIRAWDataset
    from monodepth2_amd.loader import BatchLoader
    ds = KITTIRAWDataset(root, lines, H, W, FRAME_IDS, S, is_train=True, img_ext=".png")
    loaders = {name: BatchLoader(ds, batch, shuffle=True, seed=0, num_workers=threads, device_png=flag)
               for name, flag in (("pil", False), ("device_png", True))}
    times = {name: [] for name in loaders}
    n = 0
    for rep in range(repeats + 1):
        for name, ld in loaders.items():
            ld.set_epoch(rep)
            t, n = epoch_time(ld)
            if rep:
                times[name].append(t)
    out = {"batch": batch, "threads": threads, "batches": n}
    for name, ld in loaders.items():
        t = statistics.median(times[name])
        out[name] = {"epoch_s": round(t, 3), "epoch_s_all": [round(x, 3) for x in times[name]],
                     "frames_per_s": round(n * batch * len(FRAME_IDS) / t, 1), "pil_fallbacks": ld.pil_fallbacks}
        ld.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[36, 256])
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree-frames", type=int, default=640)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--segment-bytes", type=int, default=png_ops.SEGMENT_BYTES, help="of the indexed sections")
    ap.add_argument("--sections", nargs="+", default=["kernel", "pillow", "pack", "loader"],
                    choices=["kernel", "pillow", "pack", "loader", "kernels", "indexed", "kernels_indexed"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "png_decode.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/png_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    frames = frames_of(max(args.frames), args.height, args.width)
    with ThreadPoolExecutor(16) as pool:
        files = list(pool.map(png_of, frames))
    if "kernels" in args.sections:
        call, _, _, _ = staged_call(files[:args.frames[0]], dev)
        call()
        call()
        torch.cuda.synchronize()
        return
    if "kernels_indexed" in args.sections:
        call = staged_call_indexed(files[:args.frames[0]], dev, args.segment_bytes)[0]
        call()
        call()
        torch.cuda.synchronize()
        return
    result = {"height": args.height, "width": args.width, "repeats": args.repeats, "synthetic_inputs": True,
              "mean_file_bytes": round(sum(map(len, files)) / len(files)), "device": torch.cuda.get_device_name(0)}
    for section in ("kernel", "pillow", "pack", "loader"):
        result[section] = "not measured"
    if "kernel" in args.sections:
        result["kernel"] = [bench_kernel(files[:n], frames[0], dev, args.repeats) for n in args.frames]
    if "pillow" in args.sections:
        result["pillow"] = bench_pillow(files[:min(max(args.frames), 64)])
    if "indexed" in args.sections:
        # LDS per workgroup of the segment kernel: (S + 264) 16-bit symbols, the 2 KiB input buffer and
        # the tables (8416 bytes with the input buffer: what png_index_kernel, which has no window, takes)
        result["indexed"] = {"segment_bytes": args.segment_bytes,
                             "segment_kernel_lds_bytes": 2 * (args.segment_bytes + 264) + 8416,
                             "kernel": [bench_indexed(files[:n], frames[0], dev, min(args.repeats, 3),
                                                      args.segment_bytes) for n in args.frames]}
        root = tempfile.mkdtemp(prefix="md2_pngbench_")
        try:
            lines, size = write_tree(root, args.tree_frames, args.height, args.width)
            result["tree"] = {"frames": args.tree_frames, "png_bytes": size}
            result["indexed"]["loader"] = bench_loader_packs(root, lines, args.batch, args.threads,
                                                             min(args.repeats, 3), dev, args.segment_bytes)
        finally:
            shutil.rmtree(root, ignore_errors=True)
    if "pack" in args.sections or "loader" in args.sections:
        root = tempfile.mkdtemp(prefix="md2_pngbench_")
        try:
            lines, size = write_tree(root, args.tree_frames, args.height, args.width)
            result["tree"] = {"frames": args.tree_frames, "png_bytes": size}
            if "pack" in args.sections:
                result["pack"] = bench_pack(root, lines, dev, min(args.repeats, 3), args.threads)
            if "loader" in args.sections:
                result["loader"] = bench_loader(root, lines, args.batch, args.threads, min(args.repeats, 3))
        finally:
            shutil.rmtree(root, ignore_errors=True)
    result["note"] = ("tools/png_bench.py on one MI355X, 16 host CPUs; kernel: device-resident streams, HIP events; "
                      "pillow: the same files decoded from memory on this host; pack and loader: end to end on PNG "
                      "files just written (page cache), both routes alternated in one run; informational")
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
