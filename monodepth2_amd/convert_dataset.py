"""Convert a KITTI tree from PNG to JPEG on the device: the reference's preparation step

    find kitti_data/ -name '*.png' | parallel 'convert -quality 92 -sampling-factor 2x2,1x1,1x1 {.}.png {.}.jpg'

as `python -m monodepth2_amd.convert_dataset --data_path ROOT [--lists FILE ...]`.

Every `.png` under --data_path (or, with --lists, every frame those split lists name, found as
`pack_dataset --png` finds them) is decoded by PIL on host threads straight into pinned
memory (with --device_png: by the device's PNG decoder, csrc/png.hip), encoded `--batch` at a time by the device encoder (csrc/jpegenc.hip) and written as
NAME.jpg beside it, through a temporary name and os.replace.  Each file is byte-equal to
`Image.open(png).convert("RGB").save(jpg, quality=Q, subsampling=S)`.  An
existing .jpg is skipped without --overwrite; --remove_png deletes a PNG only once its .jpg
is in place (the default keeps it, unlike the reference's one-liner with `&& rm`).
"""
from __future__ import annotations

import argparse
import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import numpy as np
from PIL import Image

from . import jpeg_ops, png_ops


def png_files(data_path: str) -> List[str]:
    """Every .png under `data_path`, sorted."""
    out = []
    for root, _, files in os.walk(data_path):
        out.extend(os.path.join(root, f) for f in files if f.lower().endswith(".png"))
    return sorted(out)


def jpg_path(png: str) -> str:
    return os.path.splitext(png)[0] + ".jpg"


def convert_files(pngs: Sequence[str], quality: int = 92, sampling="4:2:0", overwrite: bool = False,
                  remove_png: bool = False, device=None, batch: int = 64, threads: int = 8,
                  device_png: bool = False) -> Dict:
    """Converts the PNG files `pngs`; returns {"frames", "converted", "skipped", "removed",
    "bytes_in", "bytes_out"} (bytes of the PNGs read and of the JPEGs written).  With
    device_png the host threads only read and parse: the files png_ops.parse_png takes are
    decoded on the device into a flat buffer that goes straight into the encoder (the frames
    never visit the host; "device_decoded" counts them), the others go through PIL as before.
    The files written are the same bytes either way."""
    stats = {"frames": len(pngs), "converted": 0, "skipped": 0, "removed": 0, "bytes_in": 0, "bytes_out": 0}
    if device_png:
        stats["device_decoded"] = 0
    todo = []
    for p in pngs:
        if not overwrite and os.path.exists(jpg_path(p)):
            stats["skipped"] += 1       # and its PNG stays: this run did not convert it
        else:
            todo.append(p)
    batch = max(int(batch), 1)

    def size(path):
        try:
            with Image.open(path) as im:
                return im.height, im.width
        except FileNotFoundError:
            raise FileNotFoundError(f"no such image file {path}") from None

    def parse(path):
        try:
            with open(path, "rb") as f:
                return png_ops.parse_png(f.read())
        except FileNotFoundError:
            raise FileNotFoundError(f"no such image file {path}") from None

    with ThreadPoolExecutor(max(threads, 1)) as pool:
        for start in range(0, len(todo), batch):
            chunk = todo[start:start + batch]
            parsed = list(pool.map(parse, chunk)) if device_png else [None] * len(chunk)
            on_device = [i for i, s in enumerate(parsed) if s is not None]
            by_pil = [i for i, s in enumerate(parsed) if s is None]
            streams = [None] * len(chunk)
            if on_device:
                flat, offsets, shapes = png_ops.decode_png_frames([parsed[i] for i in on_device], device,
                                                                  names=[chunk[i] for i in on_device])
                encoded = jpeg_ops.encode_jpeg_batch(flat, quality=quality, sampling=sampling, device=device,
                                                     check=True, offsets=offsets, sizes=shapes)
                for i, s in zip(on_device, encoded):
                    streams[i] = s
                stats["device_decoded"] += len(on_device)
            if by_pil:
                sizes = list(pool.map(size, [chunk[i] for i in by_pil]))

                def fill(k, dest):
                    with Image.open(chunk[by_pil[k]]) as im:
                        dest[...] = np.asarray(im.convert("RGB"))

                encoded = jpeg_ops.encode_jpeg_batch(sizes, quality=quality, sampling=sampling, device=device,
                                                     check=True, fill=fill, pool=pool)
                for i, s in zip(by_pil, encoded):
                    streams[i] = s

            def write(i):
                data = jpeg_ops.jpeg_file_bytes(streams[i])     # the stuffing, then the file
                out = jpg_path(chunk[i])
                tmp = out + ".tmp"
                try:
                    with open(tmp, "wb") as f:
                        f.write(data)
                    os.replace(tmp, out)
                finally:
                    if os.path.exists(tmp):
                        os.remove(tmp)
                nin = os.path.getsize(chunk[i])
                if remove_png:
                    os.remove(chunk[i])
                return nin, len(data)

            for nin, nout in pool.map(write, range(len(chunk))):
                stats["converted"] += 1
                stats["removed"] += 1 if remove_png else 0
                stats["bytes_in"] += nin
                stats["bytes_out"] += nout
    return stats


def main(argv: Optional[Sequence[str]] = None):
    from .datasets import DATASETS, readlines
    ap = argparse.ArgumentParser(description="Convert a dataset's PNG frames to JPEG on the device (MI355X build)")
    ap.add_argument("--data_path", required=True, help="dataset root, as for train")
    ap.add_argument("--lists", nargs="+", default=None, help="convert only the frames these split lists name")
    ap.add_argument("--dataset", default="kitti", choices=sorted(DATASETS))
    ap.add_argument("--frame_ids", nargs="+", type=int, default=[0, -1, 1])
    ap.add_argument("--use_stereo", action="store_true", help="also the other camera of every line")
    ap.add_argument("--quality", type=int, default=92)
    ap.add_argument("--sampling", default="420", choices=["444", "422", "420"])
    ap.add_argument("--remove_png", action="store_true", help="delete a PNG once its .jpg is in place")
    ap.add_argument("--overwrite", action="store_true", help="convert also where a .jpg exists")
    ap.add_argument("--batch", type=int, default=64, help="frames encoded per device call")
    ap.add_argument("--threads", type=int, default=8, help="host threads decoding and writing (at most 16)")
    ap.add_argument("--device_png", action="store_true",
                    help="decode 8-bit RGB PNG files on the GPU too (HIP kernels, bit-equal to PIL): the frames go "
                         "from the decoder to the encoder without visiting the host; other files go through PIL")
    args = ap.parse_args(argv)
    jpeg_ops.quality_tables(args.quality)       # refuses a quality outside 1..100 before anything is read
    if args.lists:
        from .pack import frame_paths
        paths = frame_paths(args.data_path, [readlines(p) for p in args.lists], args.dataset, True, args.frame_ids,
                            args.use_stereo)
        pngs = sorted(paths.values())
    else:
        pngs = png_files(args.data_path)
    stats = convert_files(pngs, args.quality, args.sampling, args.overwrite, args.remove_png, batch=args.batch,
                          threads=min(max(args.threads, 1), 16), device_png=args.device_png)
    print(json.dumps(stats))
    return stats


if __name__ == "__main__":
    main()
