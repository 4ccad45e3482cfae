"""Input pipeline timing: the mixed-size augment against the single-size one, and the
batch loader end to end on JPEG files (informational, like tools/velo_bench.py).

    python tools/loader_bench.py [--batch 12] [--repeats 5] [--calls 20] [--frames 160]
                                 [--threads 1 8 16] [--out profiles/loader_bench.json]
                                 [--device_decode] [--subsampling 4:2:0 4:2:2]
                                 [--pack] [--sections augment loader decode]

augment   md2_aug_run_mixed on --batch items x 3 frames that mix KITTI raw's four decoded
          sizes (375x1242, 370x1226, 374x1238, 376x1241, a quarter of the items each)
          against md2_aug_run2 of a single-size plan on --batch x 3 frames of 375x1242,
          both to the 192x640 four-level pyramid with mixed draws; frames resident on the
          device.  HIP events around --calls calls, alternating the two, one warm-up
          each, the median of --repeats.
loader    loader.BatchLoader over a synthetic KITTI-raw tree (four drives, one per size,
          --frames JPEG frames each, written with PIL at quality 92 from textured noise),
          frame ids [0, -1, 1], shuffled, decoded by 1 / 8 / 16 threads: wall time of one
          whole epoch, through the last batch's device synchronise, one warm-up epoch, the
          median of --repeats; frames per second = decoded JPEG files per second.

jpeg      with --device_decode: the loader section is measured per --subsampling (the tree
          is written at 4:2:0, PIL's default and what this tool always wrote, or at 4:2:2,
          KITTI's own) and per thread count for BOTH paths in one run, alternating an epoch
          of the PIL path (device_decode=False: untouched code, the baseline) with an epoch
          of the device path over the same tree, one warm-up epoch each; and HIP events
          around --calls jpeg_ops.decode_jpeg_batch calls on 36 frames of 375x1242 (host
          staging included in what the events see only as far as it delays the launches;
          the wall time per call is reported beside it).  Never more than 16 threads.

pack      with --pack (implies --device_decode): the tree is packed once with
          pack.build_pack and a third path, BatchLoader(pack=...), alternates epoch by epoch
          with the PIL path and the --device_decode path from disk (both untouched code: the
          baselines) in the same run; the pack's size relative to the JPEG files is
          reported.  The decode section then alternates --calls decode_jpeg_batch calls with
          --calls decode_jpeg_batch_indexed calls on the same 36 frames in one process, HIP
          events and wall time for each.  `--sections decode --calls 1 --repeats 1` under a
          kernel trace gives the per-kernel split of both chains.

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monodepth2_amd.augment import GpuAugment, GpuAugmentMixed, draw_item, pack_items, pack_ragged  # noqa: E402
from monodepth2_amd.datasets import KITTIRAWDataset  # noqa: E402
from monodepth2_amd.jpeg_ops import (decode_jpeg_batch, decode_jpeg_batch_indexed, describe_batch,  # noqa: E402
                                     describe_batch_indexed, index_jpeg_batch, index_nsub, parse_jpeg)
from monodepth2_amd.loader import BatchLoader  # noqa: E402
from monodepth2_amd.pack import FramePack, build_pack  # noqa: E402

SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}

SIZES = [(375, 1242), (370, 1226), (374, 1238), (376, 1241)]
H, W, S = 192, 640, 4
FRAME_IDS = [0, -1, 1]


def texture(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.zeros((h, w, 3))
    for _ in range(6):
        k = rng.uniform(0.005, 0.05, 2)
        base += rng.uniform(20, 60) * np.sin(k[0] * xx + k[1] * yy + rng.uniform(0, 6.3))[..., None] \
            * rng.uniform(0.3, 1.0, 3)
    base += 128 + rng.normal(0, 12, base.shape)
    return np.clip(base, 0, 255).astype(np.uint8)


def bench_augment(batch, calls, repeats):
    rng = np.random.default_rng(0)
    draws = [draw_item(random.Random(i)) for i in range(batch)]
    items = pack_items(draws)
    F = len(FRAME_IDS)
    one = [texture(rng, h, w) for h, w in SIZES]
    mixed_frames = [[one[b % len(SIZES)] for b in range(batch)] for _ in range(F)]
    buf, offs, sizes = pack_ragged(mixed_frames)
    ragged = torch.from_numpy(buf).cuda()
    dense = torch.from_numpy(np.broadcast_to(one[0], (F, batch) + one[0].shape).copy()).cuda()
    mixed = GpuAugmentMixed(H, W, FRAME_IDS, batch, S, sizes=SIZES)
    single = GpuAugment(H, W, SIZES[0][0], SIZES[0][1], FRAME_IDS, batch, S)
    runs = {"mixed": lambda: mixed.run(ragged, sizes, offs, items), "single": lambda: single.run(dense, items)}
    times = {k: [] for k in runs}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / calls)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"batch": batch, "frames": F, "calls": calls, "mixed_ms": med["mixed"], "single_ms": med["single"],
            "ratio": med["mixed"] / med["single"], "mixed_ms_all": times["mixed"], "single_ms_all": times["single"],
            "classes_present": len(set(sizes))}


def write_tree(root, frames, subsampling="4:2:0"):
    rng = np.random.default_rng(1)
    lines = []
    for n, (h, w) in enumerate(SIZES):
        drive = "2011_09_{:02d}/2011_09_{:02d}_drive_0001_sync".format(26 + n, 26 + n)
        folder = os.path.join(root, drive, "image_02/data")
        os.makedirs(folder)
        base = [texture(rng, h, w) for _ in range(4)]
        for f in range(frames):
            Image.fromarray(np.roll(base[f % 4], 3 * f, axis=1)).save(
                os.path.join(folder, "{:010d}.jpg".format(f)), quality=92, subsampling=SUBSAMPLING[subsampling])
        lines += ["{} {} l".format(drive, f) for f in range(1, frames - 1)]
    return lines


def epoch_time(ld):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for batch_inputs in ld:
        n += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, n


def bench_loader(batch, frames, threads_list, repeats, subsampling="4:2:0", device_decode=False, pack=False):
    """Epoch times per thread count; with device_decode both paths, with pack all three,
    alternated epoch by epoch."""
    out = {}
    paths = [("pil", False), ("device", True)] if device_decode or pack else [("pil", False)]
    with tempfile.TemporaryDirectory() as root, tempfile.TemporaryDirectory() as pack_dir:
        lines = write_tree(root, frames, subsampling)
        size = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(root) for f in fs)
        ds = KITTIRAWDataset(root, lines, H, W, FRAME_IDS, S, is_train=True, img_ext=".jpg")
        packed = None
        if pack:
            t0 = time.perf_counter()
            stats = build_pack(os.path.join(pack_dir, "tree.pack"), root, [lines], frame_ids=FRAME_IDS, threads=16)
            out["pack"] = dict(stats, build_s=time.perf_counter() - t0,
                               pack_over_files=stats["pack_bytes"] / stats["file_bytes"])
            packed = FramePack(os.path.join(pack_dir, "tree.pack"))
        for threads in threads_list:
            threads = min(threads, 16)
            loaders = {name: BatchLoader(ds, batch, shuffle=True, seed=0, num_workers=threads, device_decode=flag)
                       for name, flag in paths}
            if packed is not None:
                loaders["pack"] = BatchLoader(ds, batch, shuffle=True, seed=0, num_workers=threads, pack=packed)
            times = {name: [] for name in loaders}
            n = 0
            for rep in range(repeats + 1):
                for name, ld in loaders.items():
                    ld.set_epoch(rep)           # the same order for both paths
                    ld.uploaded_bytes = 0
                    t, n = epoch_time(ld)
                    if rep:
                        times[name].append(t)
            row = {}
            for name, ld in loaders.items():
                t = statistics.median(times[name])
                row[name] = {"epoch_s": t, "batches": n, "frames_per_s": n * batch * len(FRAME_IDS) / t,
                             "items_per_s": n * batch / t, "epoch_s_all": times[name],
                             "uploaded_bytes_per_batch": ld.uploaded_bytes / max(n, 1)}
                ld.close()
            out[str(threads)] = row if device_decode or pack else row["pil"]
            print("loader {} threads {}: {}".format(subsampling, threads, {k: round(v["items_per_s"]) for k, v in
                                                                          row.items()}), file=sys.stderr, flush=True)
        out["files"] = len(SIZES) * frames
        out["mean_file_bytes"] = size / (len(SIZES) * frames)
        out["subsampling"] = subsampling
    return out


def bench_decode(calls, repeats, subsampling, frames=36):
    """HIP events (and wall time) around `calls` decode_jpeg_batch calls on `frames` frames."""
    import io
    rng = np.random.default_rng(2)
    streams = []
    for _ in range(4):
        buf = io.BytesIO()
        Image.fromarray(texture(rng, *SIZES[0])).save(buf, "JPEG", quality=92, subsampling=SUBSAMPLING[subsampling])
        streams.append(parse_jpeg(buf.getvalue()))
    streams = [streams[i % 4] for i in range(frames)]
    per = (SIZES[0][0] * SIZES[0][1] * 3 + 255) // 256 * 256
    offsets = [i * per for i in range(frames)]
    out = torch.empty(frames * per, dtype=torch.uint8, device="cuda")
    decode_jpeg_batch(streams, out, offsets, check=True)
    ms, wall = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(calls):
            decode_jpeg_batch(streams, out, offsets)
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / calls)
        ms.append(a.elapsed_time(b) / calls)
    return {"frames": frames, "size": list(SIZES[0]), "subsampling": subsampling, "calls": calls,
            "ms_per_call": statistics.median(ms), "ms_per_call_all": ms, "wall_ms_per_call": statistics.median(wall),
            "frames_per_s": frames / (statistics.median(ms) * 1e-3),
            "uploaded_bytes_per_batch": describe_batch(streams, offsets)[4],
            "decoded_bytes_per_batch": frames * SIZES[0][0] * SIZES[0][1] * 3}


def bench_decode_indexed(calls, repeats, subsampling, frames=36):
    """HIP events (and wall time) around `calls` decode_jpeg_batch calls and `calls`
    decode_jpeg_batch_indexed calls on the same `frames` frames, alternated in one process;
    the first is the baseline (untouched code)."""
    import io
    rng = np.random.default_rng(2)
    streams = []
    for _ in range(4):
        buf = io.BytesIO()
        Image.fromarray(texture(rng, *SIZES[0])).save(buf, "JPEG", quality=92, subsampling=SUBSAMPLING[subsampling])
        streams.append(parse_jpeg(buf.getvalue()))
    streams = [streams[i % 4] for i in range(frames)]
    four = index_jpeg_batch(streams[:4], "cuda", check=True)
    indexes = [four[i % 4] for i in range(frames)]
    per = (SIZES[0][0] * SIZES[0][1] * 3 + 255) // 256 * 256
    offsets = [i * per for i in range(frames)]
    out = torch.zeros(frames * per, dtype=torch.uint8, device="cuda")   # zeros: the gaps between frames are compared too
    ref = torch.zeros_like(out)
    runs = {"sync": lambda o=out: decode_jpeg_batch(streams, o, offsets),
            "indexed": lambda o=out: decode_jpeg_batch_indexed(streams, indexes, o, offsets)}
    decode_jpeg_batch(streams, ref, offsets, check=True)          # warm-up of both, and the same bytes
    decode_jpeg_batch_indexed(streams, indexes, out, offsets, check=True)
    same = bool(torch.equal(out, ref))
    ms, wall = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(repeats):
        for name, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3 / calls)
            ms[name].append(a.elapsed_time(b) / calls)
    res = {"frames": frames, "size": list(SIZES[0]), "subsampling": subsampling, "calls": calls, "bit_equal": same,
           "subsequences_per_frame": sum(index_nsub(len(s.data)) for s in streams) / frames}
    for name in runs:
        res[name] = {"ms_per_call": statistics.median(ms[name]), "ms_per_call_all": ms[name],
                     "wall_ms_per_call": statistics.median(wall[name]),
                     "frames_per_s": frames / (statistics.median(ms[name]) * 1e-3)}
    res["sync"]["uploaded_bytes_per_batch"] = describe_batch(streams, offsets)[4]
    res["indexed"]["uploaded_bytes_per_batch"] = describe_batch_indexed(streams, offsets)[5]
    res["indexed_over_sync"] = res["indexed"]["ms_per_call"] / res["sync"]["ms_per_call"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--threads", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--out", type=str)
    ap.add_argument("--device_decode", action="store_true", help="also measure the device JPEG decoder, "
                                                                 "alternated with the PIL path in the same run")
    ap.add_argument("--subsampling", nargs="+", default=["4:2:0"], choices=["4:2:0", "4:2:2"],
                    help="chroma subsampling of the synthetic tree (4:2:0 is what PIL writes by default, "
                         "4:2:2 what KITTI's files have)")
    ap.add_argument("--pack", action="store_true", help="also measure the packed frame file: loader epochs "
                                                        "alternated with the PIL and --device_decode paths, "
                                                        "and the indexed decoder alternated with the unindexed")
    ap.add_argument("--sections", nargs="+", default=["augment", "loader", "decode"],
                    choices=["augment", "loader", "decode"], help="what to measure (all by default)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench needs a GPU: nothing here is timed on the host alone")
    res = {"tool": "loader_bench", "device": torch.cuda.get_device_name(0),
           "python": platform.python_version(), "pillow": Image.__version__}
    if "augment" in args.sections:
        res["augment"] = bench_augment(args.batch, args.calls, args.repeats)
    if args.pack:
        if "loader" in args.sections:
            res["loader_pack"] = {sub: bench_loader(args.batch, args.frames, args.threads, args.repeats, sub, True, True)
                                  for sub in args.subsampling}
        if "decode" in args.sections:
            res["decode_pack"] = {sub: bench_decode_indexed(args.calls, args.repeats, sub) for sub in args.subsampling}
    elif args.device_decode:
        if "loader" in args.sections:
            res["loader_jpeg"] = {sub: bench_loader(args.batch, args.frames, args.threads, args.repeats, sub, True)
                                  for sub in args.subsampling}
        if "decode" in args.sections:
            res["decode"] = {sub: bench_decode(args.calls, args.repeats, sub) for sub in args.subsampling}
    elif "loader" in args.sections:
        res["loader"] = bench_loader(args.batch, args.frames, args.threads, args.repeats, args.subsampling[0])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
