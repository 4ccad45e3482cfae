"""Capture tests/golden/dataset/dataset_paths.json from the reference's own dataset
classes (datasets/mono_dataset.py, datasets/kitti_dataset.py), unmodified, on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/dataset/make_dataset_golden.py [--ref /root/reference]

`torchvision` and `skimage` are not installed: both are stubbed in `sys.modules` before
the import (Resize / ToTensor / ColorJitter.get_params become no-ops; no image is
processed here), `Image.ANTIALIAS` (gone from Pillow 10) is set to LANCZOS and `np.int`
to `int`.  Each dataset's `loader` is replaced by one that records the path it is asked
for and returns a 2 x 2 image, and `get_color` is wrapped to record the side and the
flip it is called with.  For every case (dataset class, frame ids, is_train, split line)
the reference's `__getitem__` runs once with `random.seed(case number)`; recorded are the
requested paths relative to the data root, the sides, the flip, and stereo_T[0, 3] when
"s" is a frame id, or the name of the exception it raised (a one-field line has no side,
and every KITTI class indexes `side_map` with it).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = "/data/kitti"

# (class, frame ids, is_train, first line (check_depth reads it), lines)
CASES = [
    ("KITTIRAWDataset", [0, -1, 1], True,
     ["2011_09_26/2011_09_26_drive_0022_sync 473 r", "2011_09_29/2011_09_29_drive_0026_sync 1 l",
      "2011_10_03/2011_10_03_drive_0034_sync 1743 l", "2011_09_30/2011_09_30_drive_0028_sync"]),
    ("KITTIRAWDataset", [0, "s"], True,
     ["2011_09_26/2011_09_26_drive_0022_sync 473 r", "2011_09_28/2011_09_28_drive_0001_sync 12 l",
      "2011_09_26/2011_09_26_drive_0005_sync 7 r", "2011_09_26/2011_09_26_drive_0005_sync 8 l"]),
    ("KITTIRAWDataset", [0, -1, 1, "s"], False,
     ["2011_09_26/2011_09_26_drive_0022_sync 473 l", "2011_09_26/2011_09_26_drive_0022_sync 474 r"]),
    ("KITTIOdomDataset", [0, -1, 1], True, ["9 1234 l", "0 3 r", "10 17 l", "4"]),
    ("KITTIOdomDataset", [0, "s"], True, ["9 1234 l", "3 5 r"]),
    ("KITTIDepthDataset", [0, -1, 1], False,
     ["2011_09_26/2011_09_26_drive_0022_sync 473 r", "2011_10_03/2011_10_03_drive_0027_sync 5 l"]),
    ("KITTIDepthDataset", [0, "s"], True,
     ["2011_09_26/2011_09_26_drive_0022_sync 473 r", "2011_10_03/2011_10_03_drive_0027_sync 5 l"]),
]


def stub_modules():
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")

    class Resize:
        def __init__(self, size, interpolation=None):
            pass

        def __call__(self, img):
            return img

    class ToTensor:
        def __call__(self, img):
            return img

    class ColorJitter:
        @staticmethod
        def get_params(brightness, contrast, saturation, hue):
            return lambda img: img

    tr.Resize, tr.ToTensor, tr.ColorJitter = Resize, ToTensor, ColorJitter
    tv.transforms = tr
    sk = types.ModuleType("skimage")
    sk.transform = types.ModuleType("skimage.transform")
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "skimage": sk,
                        "skimage.transform": sk.transform})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "dataset_paths.json"))
    args = ap.parse_args()
    from PIL import Image
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS
    np.int = int
    stub_modules()
    sys.path.insert(0, args.ref)
    import datasets as ref

    out = []
    for n, (cls, frame_idxs, is_train, lines) in enumerate(CASES):
        ds = getattr(ref, cls)(ROOT, lines, 192, 640, frame_idxs, 4, is_train=is_train, img_ext=".png")
        asked, calls = [], []
        ds.loader = lambda path: (asked.append(os.path.relpath(path, ROOT)), Image.new("RGB", (2, 2)))[1]
        get_color = ds.get_color

        def recording(folder, frame_index, side, do_flip):
            calls.append((side, bool(do_flip)))
            return get_color(folder, frame_index, side, do_flip)

        ds.get_color = recording
        ds.load_depth = False
        items = []
        for i, line in enumerate(lines):
            del asked[:], calls[:]
            random.seed(n * 100 + i)
            rec = {"line": line}
            try:
                item = ds[i]
                rec["paths"] = list(asked)
                rec["sides"] = [c[0] for c in calls]
                rec["do_flip"] = calls[0][1]
                assert all(c[1] == calls[0][1] for c in calls)
                if "s" in frame_idxs:
                    rec["stereo_tx"] = float(np.asarray(item["stereo_T"])[0, 3])
            except (KeyError, IndexError, ValueError) as e:
                rec["error"] = type(e).__name__
            items.append(rec)
        out.append({"dataset": cls, "frame_idxs": frame_idxs, "is_train": is_train, "img_ext": ".png",
                    "K": np.asarray(ds.K).tolist(), "full_res_shape": list(ds.full_res_shape),
                    "side_map": ds.side_map, "items": items})
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(args.out, os.path.getsize(args.out), "bytes,", sum(len(c["items"]) for c in out), "lines")


if __name__ == "__main__":
    main()
