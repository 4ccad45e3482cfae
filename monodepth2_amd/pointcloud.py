"""Point clouds from single-image depth predictions, on the device.

    python -m monodepth2_amd.pointcloud --image_path FILE_OR_DIR --load_weights_folder DIR \\
        [--ext jpg] [--num_layers 18] [--pred_metric_depth] [--intrinsics FX FY CX CY] \\
        [--stride 1] [--near 1e-3] [--far 80] [--poses poses.npy --out cloud.ply]

The networks run as in `infer` (`infer.load_networks`, `infer.preprocess`,
`evaluate_depth.predict_disparities`), sorted files in chunks of 16.  The map of an image is
its disparity resized to the image's own size — the `resized` output of
`viz_ops.colorize_disparity`, what the reference's picture is made from — and the colours
are the image's own bytes.  `points_ops.depth_to_points` (disp_to_depth with 0.1 and 100,
BackprojectDepth, range filter, compaction, PLY records) makes the file bodies, one call per
group of equally sized images.

--intrinsics are normalised as the reference's K is (default KITTI's 0.58 1.92 0.5 0.5,
datasets.KITTIDataset.K): rows 0 and 1 are scaled by the image's width and height and
inv_K = np.linalg.pinv(K) on the float32 matrix, as mono_dataset.py builds it.
--pred_metric_depth scales depth by STEREO_SCALE_FACTOR (stereo-trained KITTI models).

Without --poses one NAME_cloud.ply is written beside each input.  With --poses FILE, the
(N-1,4,4) float32 array `evaluate_pose` saves for the N sorted images (all of one size),
every image's points are moved to the first camera's frame with the reference's dump_xyz
rule (evaluate_pose.py:23-30): C_0 = I, C_{i+1} = C_i . P_i, chained on the host in fp64 and
handed to the operator as float32; one fused file is written at --out.

--model_name and its download are deliberately absent, as in `infer`; there is no CPU path.
"""
from __future__ import annotations

import argparse
import glob
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import PIL.Image as pil
import torch

from . import infer
from .datasets import KITTIDataset
from .evaluate_depth import STEREO_SCALE_FACTOR, predict_disparities
from .points_ops import RECORD_BYTES, depth_to_points, write_ply
from .viz_ops import colorize_disparity

DEFAULT_INTRINSICS = tuple(float(KITTIDataset.K[i, j]) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))


def inverse_intrinsics(intrinsics: Sequence[float], height: int, width: int) -> np.ndarray:
    """The (4,4) float32 inv_K of an image size from normalised fx, fy, cx, cy
    (mono_dataset.py:157-165 at scale 0)."""
    fx, fy, cx, cy = intrinsics
    K = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    K[0, :] *= width
    K[1, :] *= height
    return np.linalg.pinv(K)


def chain_poses(poses: np.ndarray) -> np.ndarray:
    """(N-1,4,4) frame-to-frame transforms -> (N,4,4) float32 camera-to-world, dump_xyz's
    rule in fp64: C_0 = I, C_{i+1} = C_i . P_i."""
    poses = np.asarray(poses)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise SystemExit("--poses must hold an (N-1,4,4) array, got shape {}".format(poses.shape))
    chain = [np.eye(4)]
    for p in poses.astype(np.float64):
        chain.append(np.dot(chain[-1], p))
    return np.stack(chain).astype(np.float32)


def check_pose_count(num_poses: int, num_images: int) -> None:
    if num_poses != num_images - 1:
        raise SystemExit("--poses holds {:d} transforms but {:d} images were found: N images need N-1 "
                         "transforms".format(num_poses, num_images))


def predict_maps(encoder, depth_decoder, images: Sequence[pil.Image], feed_hw: Sequence[int]):
    """One pass of the networks on a chunk; per group of equally sized images (size ->
    (indices, resized (n,H,W) float32 on the device)): the disparities at the images' sizes."""
    device = next(encoder.parameters()).device
    x = torch.cat([infer.preprocess(im, feed_hw, device) for im in images])
    disp = predict_disparities(encoder, depth_decoder, x)
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, im in enumerate(images):
        groups.setdefault((im.height, im.width), []).append(i)
    out = {}
    for size, idx in groups.items():
        sel = disp if len(idx) == len(images) else disp[torch.as_tensor(idx, device=device)]
        _, resized = colorize_disparity(sel, size, return_resized=True)
        out[size] = (idx, resized)
    return out


def clouds_of(resized: torch.Tensor, images: Sequence[pil.Image], args, T: Optional[np.ndarray] = None):
    """depth_to_points on one group: (vertices bytes on the host, offsets (n+1) on the host)."""
    device = resized.device
    n, H, W = resized.shape
    rgb = torch.from_numpy(np.stack([np.asarray(im, dtype=np.uint8) for im in images])).to(device)
    inv_K = torch.from_numpy(inverse_intrinsics(args.intrinsics, H, W)).to(device).expand(n, 4, 4).contiguous()
    Td = torch.from_numpy(np.ascontiguousarray(T, dtype=np.float32)).to(device) if T is not None else None
    vertices, offsets = depth_to_points(resized, rgb, inv_K, Td, min_depth=0.1, max_depth=100.0,
                                        depth_scale=STEREO_SCALE_FACTOR if args.pred_metric_depth else 1.0,
                                        near=args.near, far=args.far, stride=args.stride)
    offsets = offsets.cpu().numpy().astype(np.int64)
    return vertices[:int(offsets[-1]) * RECORD_BYTES].cpu().numpy(), offsets


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Point clouds (binary PLY) from single-image depth predictions.")
    parser.add_argument("--image_path", type=str, required=True, help="path to a test image or folder of images")
    parser.add_argument("--load_weights_folder", type=str, required=True,
                        help="checkpoint folder with encoder.pth and depth.pth")
    parser.add_argument("--ext", type=str, default="jpg", help="image extension to search for in folder")
    parser.add_argument("--num_layers", type=int, default=18, choices=[18, 34, 50, 101, 152])
    parser.add_argument("--pred_metric_depth", action="store_true",
                        help="scale depth by STEREO_SCALE_FACTOR (this only makes sense for stereo-trained KITTI "
                             "models)")
    parser.add_argument("--intrinsics", type=float, nargs=4, default=list(DEFAULT_INTRINSICS),
                        metavar=("FX", "FY", "CX", "CY"),
                        help="normalised by the image width (fx, cx) and height (fy, cy); default KITTI's")
    parser.add_argument("--stride", type=int, default=1, help="keep every stride-th row and column")
    parser.add_argument("--near", type=float, default=1e-3, help="nearest z kept (inclusive)")
    parser.add_argument("--far", type=float, default=80.0, help="farthest z kept (inclusive)")
    parser.add_argument("--poses", type=str, help="(N-1,4,4) float32 poses.npy of evaluate_pose for the N sorted "
                                                  "images: one fused cloud in the first camera's frame")
    parser.add_argument("--out", type=str, help="the fused file (with --poses)")
    args = parser.parse_args(argv)
    if bool(args.poses) != bool(args.out):
        parser.error("--poses and --out go together")
    if args.stride < 1:
        parser.error("--stride must be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("monodepth2_amd.pointcloud needs a GPU (HIP kernels, no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    folder = os.path.expanduser(args.load_weights_folder)
    if not os.path.isdir(folder):
        raise SystemExit("Cannot find a folder at {}".format(folder))
    if os.path.isfile(args.image_path):
        paths = [args.image_path]
        output_directory = os.path.dirname(args.image_path)
    elif os.path.isdir(args.image_path):
        paths = sorted(glob.glob(os.path.join(args.image_path, "*.{}".format(args.ext))))
        output_directory = args.image_path
    else:
        raise SystemExit("Can not find args.image_path: {}".format(args.image_path))
    paths = [p for p in paths if not p.endswith("_disp.jpg")]   # infer's pictures are not inputs
    chain = None
    if args.poses:
        poses = np.load(args.poses)
        check_pose_count(int(poses.shape[0]) if poses.ndim else 0, len(paths))
        chain = chain_poses(poses)
    print("-> Loading model from ", folder)
    encoder, depth_decoder, feed_hw = infer.load_networks(folder, args.num_layers, device)
    print("-> Making point clouds of {:d} images".format(len(paths)))

    bodies, total, first_size = [], 0, None
    for start in range(0, len(paths), infer.BATCH):
        chunk = paths[start:start + infer.BATCH]
        images = [pil.open(p).convert("RGB") for p in chunk]
        if chain is not None:
            sizes = {(im.height, im.width) for im in images} | ({first_size} if first_size else set())
            if len(sizes) != 1:
                raise SystemExit("--poses needs images of one size, found {}".format(sorted(sizes)))
            first_size = next(iter(sizes))
        for size, (idx, resized) in predict_maps(encoder, depth_decoder, images, feed_hw).items():
            T = chain[[start + i for i in idx]] if chain is not None else None
            body, offsets = clouds_of(resized, [images[i] for i in idx], args, T)
            if chain is not None:
                bodies.append(body)
                total += int(offsets[-1])
                continue
            for j, i in enumerate(idx):
                name = os.path.splitext(os.path.basename(chunk[i]))[0]
                ply = os.path.join(output_directory, "{}_cloud.ply".format(name))
                lo, hi = int(offsets[j]), int(offsets[j + 1])
                write_ply(ply, body[lo * RECORD_BYTES:hi * RECORD_BYTES], hi - lo)
                print("   Processed {:d} of {:d} images - {:d} points in {}".format(start + i + 1, len(paths),
                                                                                   hi - lo, ply))
    if chain is not None:
        write_ply(args.out, np.concatenate(bodies) if bodies else np.zeros(0, np.uint8), total)
        print("   Fused {:d} images - {:d} points in {}".format(len(paths), total, args.out))
    print("-> Done!")


if __name__ == "__main__":
    main()
