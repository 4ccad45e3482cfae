"""Pack a KITTI tree once: `python -m monodepth2_amd.pack_dataset --data_path ROOT --lists
train_files.txt val_files.txt ... --out FILE`.

Reads the split lists, names their frames as `train` / `evaluate_depth` / `evaluate_pose`
would (--dataset, --png, --frame_ids and --use_stereo as there), and writes the frame pack
`--pack FILE` of those commands reads (pack.py).  Needs the GPU: the
synchronisation indexes are computed by the device decoder's own kernel.  With --png
--transcode [--quality 92] [--sampling 420] the PNG frames are encoded as JPEG on the device
(csrc/jpegenc.hip) instead of stored decoded: the pack `convert_dataset` followed by
`pack_dataset` would give, without writing the .jpg files; with --device_png on top the PNG
files are decoded on the device as well (csrc/png.hip), the same pack.  With
--png --png_records [--segment_bytes 16384] the 8-bit RGB PNG frames are kept as they are,
lossless and at the files' own size, each with a segment index the device decodes it from in
parallel; --png_records and --transcode exclude each other.
"""
from __future__ import annotations

import argparse
import json
from typing import Optional, Sequence

from .datasets import DATASETS, readlines
from .pack import build_pack
from .png_ops import SEGMENT_BYTES


def main(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(description="Write a frame pack for --pack (MI355X build)")
    ap.add_argument("--data_path", required=True, help="dataset root, as for train")
    ap.add_argument("--lists", nargs="+", required=True, help="split list files whose frames to pack")
    ap.add_argument("--out", required=True, help="the pack to write")
    ap.add_argument("--dataset", default="kitti", choices=sorted(DATASETS))
    ap.add_argument("--png", action="store_true", help="the tree holds png files")
    ap.add_argument("--frame_ids", nargs="+", type=int, default=[0, -1, 1])
    ap.add_argument("--use_stereo", action="store_true", help="also pack the other camera of every line")
    ap.add_argument("--transcode", action="store_true",
                    help="encode files the device decoder does not take (PNG) as JPEG on the device instead of "
                         "storing them decoded: a much smaller pack, lossy like convert_dataset")
    ap.add_argument("--quality", type=int, default=92, help="of --transcode")
    ap.add_argument("--sampling", default="420", choices=["444", "422", "420"], help="of --transcode")
    ap.add_argument("--device_png", action="store_true",
                    help="with --png --transcode: decode the 8-bit RGB PNG files on the GPU too (HIP kernels, "
                         "bit-equal to PIL), so the frames go from decoder to encoder without visiting the host")
    ap.add_argument("--png_records", action="store_true",
                    help="with --png: keep the 8-bit RGB PNG files lossless as PNG records (the deflate stream and "
                         "its segment index) instead of storing them decoded; not with --transcode")
    ap.add_argument("--segment_bytes", type=int, default=SEGMENT_BYTES,
                    help="of --png_records: output bytes per segment of the index, a power of two in 1024..32768")
    ap.add_argument("--batch", type=int, default=64, help="files indexed per device call")
    ap.add_argument("--threads", type=int, default=8, help="host threads reading and parsing files (at most 16)")
    args = ap.parse_args(argv)
    if args.png_records and args.transcode:
        ap.error("--png_records and --transcode exclude each other")
    stats = build_pack(args.out, args.data_path, [readlines(p) for p in args.lists], dataset=args.dataset,
                       png=args.png, frame_ids=args.frame_ids, use_stereo=args.use_stereo, batch=args.batch,
                       threads=min(max(args.threads, 1), 16),
                       transcode=(args.quality, args.sampling) if args.transcode else None,
                       device_png=args.device_png, png_records=args.png_records, segment_bytes=args.segment_bytes)
    stats["out"] = args.out
    print(json.dumps(stats))
    return stats


if __name__ == "__main__":
    main()
