"""Export the ground-truth depth maps of a KITTI test split (the reference's
export_gt_depth.py) as the `gt_depths.npz` that evaluate_depth.py loads.

    python -m monodepth2_amd.export_gt_depth --data_path KITTI_RAW --split eigen \\
        --split_file test_files.txt [--output gt_depths.npz] [--batch_size 16]

`eigen`: every line `<date>/<drive> <frame> <side>` of the split file names a velodyne
scan; the scans are projected into camera 2 with the points' own forward distance as the
depth (kitti_utils.generate_depth_map(..., 2, True)), `--batch_size` frames per launch
chain of the HIP operator (csrc/velo.hip).  `eigen_benchmark`: the improved ground truth's
16-bit PNGs divided by 256, on the host.  This tree ships no split lists: `--split_file`
defaults to splits/<split>/test_files.txt beside this package, and `--output` to
gt_depths.npz beside the split file.  The file's `data` is float32 (N, H, W) when all
frames share a size, else an object array of (H, W) maps (numpy 2 refuses the ragged
np.array of the reference).
"""
from __future__ import annotations

import argparse
import os
from typing import List

import numpy as np

SPLITS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "splits")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="export_gt_depth")
    ap.add_argument("--data_path", type=str, required=True, help="path to the root of the KITTI data")
    ap.add_argument("--split", type=str, required=True, choices=["eigen", "eigen_benchmark"],
                    help="which split to export gt from")
    ap.add_argument("--split_file", type=str, default=None,
                    help="the split's test_files.txt (default: splits/<split>/test_files.txt in the package)")
    ap.add_argument("--output", type=str, default=None, help="default: gt_depths.npz beside the split file")
    ap.add_argument("--batch_size", type=int, default=16, help="frames per launch chain (eigen)")
    return ap.parse_args(argv)


def read_split(path: str):
    if not os.path.isfile(path):
        raise SystemExit("Cannot find the split file {} (this tree ships no split lists: set --split_file)".format(path))
    with open(path, "r") as f:
        lines = f.read().splitlines()
    frames = []
    for line in lines:
        if not line.strip():
            continue
        folder, frame_id = line.split()[:2]
        frames.append((folder, int(frame_id)))
    return frames


def stack_maps(maps: List[np.ndarray]) -> np.ndarray:
    if len({m.shape for m in maps}) <= 1:
        return np.stack(maps).astype(np.float32) if maps else np.zeros((0, 0, 0), dtype=np.float32)
    data = np.empty(len(maps), dtype=object)
    for i, m in enumerate(maps):
        data[i] = m
    return data


def export_gt_depths_kitti(opt) -> str:
    split_file = opt.split_file or os.path.join(SPLITS_DIR, opt.split, "test_files.txt")
    frames = read_split(split_file)
    if opt.batch_size < 1:
        raise SystemExit("--batch_size must be positive")
    output = opt.output or os.path.join(os.path.dirname(os.path.abspath(split_file)), "gt_depths.npz")
    print("Exporting ground truth depths for {}".format(opt.split))
    maps: List[np.ndarray] = []
    if opt.split == "eigen":
        from .kitti_utils import generate_depth_maps
        jobs = [(os.path.join(opt.data_path, folder.split("/")[0]),
                 os.path.join(opt.data_path, folder, "velodyne_points/data", "{:010d}.bin".format(frame_id)))
                for folder, frame_id in frames]
        for calib_dir, scan in jobs:
            if not os.path.isfile(scan):
                raise SystemExit("Cannot find the velodyne scan {}".format(scan))
        for i in range(0, len(jobs), opt.batch_size):
            maps.extend(m.cpu().numpy() for m in generate_depth_maps(jobs[i:i + opt.batch_size], cam=2, vel_depth=True))
    else:
        import PIL.Image as pil
        for folder, frame_id in frames:
            path = os.path.join(opt.data_path, folder, "proj_depth", "groundtruth", "image_02",
                                "{:010d}.png".format(frame_id))
            if not os.path.isfile(path):
                raise SystemExit("Cannot find the ground-truth image {}".format(path))
            maps.append(np.array(pil.open(path)).astype(np.float32) / 256)
    print("Saving to {}".format(output))
    np.savez_compressed(output, data=stack_maps(maps))
    return output


if __name__ == "__main__":
    export_gt_depths_kitti(parse_args())
