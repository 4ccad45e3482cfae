"""KITTI raw-data helpers: calibration files, velodyne scans and the sparse depth maps the
evaluation uses as ground truth (the reference's kitti_utils.py), with the projection and
the duplicate resolution on the device (velo_ops.project_velodyne, csrc/velo.hip).

`generate_depth_map` keeps the reference's signature and returns what its function
returns, as float32 (what export_gt_depth.py stores); `generate_depth_maps` is the batched
form that leaves the maps on the device, where `eval_ops.depth_metrics` reads them.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .velo_ops import project_velodyne

_NUMERIC = frozenset("0123456789.e+- ")


def read_calib_file(path: str) -> Dict[str, object]:
    """A KITTI calibration file as {key: value}: `key: v v v` lines become float64 arrays
    when every character of the value is numeric, and stay strings otherwise (dates)."""
    out: Dict[str, object] = {}
    with open(path, "r") as f:
        for line in f:
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            value = value.strip()
            out[key] = value
            if value and _NUMERIC.issuperset(value):
                try:
                    out[key] = np.array([float(v) for v in value.split(" ")], dtype=np.float64)
                except ValueError:
                    pass
    return out


def load_velodyne_points(filename: str) -> np.ndarray:
    """A velodyne .bin scan as float32 (N, 4): forward, left, up, and 1 in place of the
    reflectance (homogeneous, like the reference)."""
    pts = np.fromfile(filename, dtype=np.float32).reshape(-1, 4)
    pts[:, 3] = 1.0
    return pts


def velo_to_image_matrix(calib_dir: str, cam: int = 2) -> Tuple[np.ndarray, Tuple[int, int]]:
    """(P, (H, W)): the fp64 3x4 matrix P_rect_0{cam} @ R_rect_00 (as 4x4) @ velo2cam (as
    4x4), multiplied left to right, and the rectified image size from S_rect_02."""
    cam2cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    velo2cam = np.eye(4)
    velo2cam[:3, :3] = velo["R"].reshape(3, 3)
    velo2cam[:3, 3] = velo["T"]
    rect = np.eye(4)
    rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    proj = cam2cam["P_rect_0%d" % cam].reshape(3, 4)
    size = cam2cam["S_rect_02"].astype(np.int32)   # width, height
    # np.dot like the reference: on one host both then give the same bits (a BLAS may fuse
    # or reorder the four-term sums, so the last bit is the host's, in either code)
    return np.dot(np.dot(proj, rect), velo2cam), (int(size[1]), int(size[0]))


def _device(device) -> torch.device:
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def generate_depth_maps(frames: Sequence[Tuple[str, str]], cam: int = 2, vel_depth: bool = False,
                        device=None) -> List[torch.Tensor]:
    """The depth maps of `frames`, a sequence of (calib_dir, velo_filename), as (H, W)
    float32 device tensors in the order given.  Frames of equal image size share one
    launch chain; calibration directories are read once.  No synchronisation."""
    device = _device(device)
    calib: Dict[str, Tuple[np.ndarray, Tuple[int, int]]] = {}
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, (calib_dir, _) in enumerate(frames):
        if calib_dir not in calib:
            calib[calib_dir] = velo_to_image_matrix(calib_dir, cam)
        groups.setdefault(calib[calib_dir][1], []).append(i)
    out: List[Optional[torch.Tensor]] = [None] * len(frames)
    for (h, w), idx in groups.items():
        scans = [np.fromfile(frames[i][1], dtype=np.float32).reshape(-1, 4) for i in idx]
        maps = depth_maps_from_arrays(scans, np.stack([calib[frames[i][0]][0] for i in idx]), h, w,
                                      vel_depth=vel_depth, device=device)
        for j, i in enumerate(idx):
            out[i] = maps[j]
    return out


def depth_maps_from_arrays(scans: Sequence[np.ndarray], P: np.ndarray, height: int, width: int,
                           vel_depth: bool = False, device=None) -> torch.Tensor:
    """Host scans ((n_b, 4) float32 each) and their (B, 3, 4) float64 matrices -> (B, H, W)
    on the device: one concatenation, three uploads, one launch chain."""
    device = _device(device)
    counts = np.zeros(len(scans) + 1, dtype=np.int64)
    np.cumsum([s.shape[0] for s in scans], out=counts[1:])
    points = np.concatenate(scans, 0) if len(scans) > 1 else np.ascontiguousarray(scans[0])
    return project_velodyne(torch.from_numpy(points).to(device, non_blocking=True),
                            torch.from_numpy(counts).to(device, non_blocking=True),
                            torch.from_numpy(np.ascontiguousarray(P, dtype=np.float64)).to(device, non_blocking=True),
                            height, width, vel_depth=vel_depth)


def generate_depth_map(calib_dir: str, velo_filename: str, cam: int = 2, vel_depth: bool = False,
                       device=None) -> np.ndarray:
    """kitti_utils.generate_depth_map of the reference: the (H, W) float32 map of one scan."""
    return generate_depth_maps([(calib_dir, velo_filename)], cam, vel_depth, device)[0].cpu().numpy()
