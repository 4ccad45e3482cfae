"""KITTI datasets: the reference's split-line rules and paths, decoding only.

Counterpart of datasets/mono_dataset.py:28-209 and datasets/kitti_dataset.py:18-134.
The constructor arguments, the split-line parsing (mono_dataset.py:143-161), `side_map`,
the three `get_image_path` forms, `check_depth`, `K` and `full_res_shape` are the
reference's.  What differs is where the work runs: `__getitem__` neither resizes nor
jitters nor flips.  It returns the decoded frames at their native size, as uint8 RGB from
`Image.open(...).convert("RGB")` (the reference's pil_loader), with the side, the size and
the item's random draws; flip, the resize pyramid, ToTensor and the colour jitter happen
on the GPU for the whole batch (augment.GpuAugmentMixed), bit-equal to the PIL pipeline.

Draws: `augment.draw_item(random.Random(item_seed(seed, epoch, index)))`, the reference's
draws in its order, but seeded per item so that a run is reproducible whatever the number
of decoding threads.  (The reference's own stream depends on its workers' seeding and
cannot be reproduced.)

This module is host-only: nothing here touches the GPU, except `KITTIRAWDataset.get_depths`,
which the loader calls once per batch on its caller's thread and stream and which projects
the velodyne scans with the HIP kernel behind `kitti_utils.generate_depth_maps`.
"""
from __future__ import annotations

import os
import random
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
from PIL import Image

from .augment import ItemDraw, draw_item


def readlines(filename: str) -> List[str]:
    """utils.py:10-15: every line of a split file."""
    with open(filename, "r") as f:
        return f.read().splitlines()


def item_seed(seed: int, epoch: int, index: int) -> int:
    """One integer per (seed, epoch, index): the seed of that item's draws."""
    return (int(seed) * 1000003 + int(epoch)) * 1000003 + int(index)


def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """Source index of every output sample of a PIL `NEAREST` resize from n_in to n_out
    (Geometry.c ImagingScaleAffine: the coordinate starts at half a step and ADVANCES by
    repeated addition in double, then truncates; a product instead lands one sample off
    where the sum's rounding crosses an integer, e.g. sample 112 of 370 -> 375)."""
    step = n_in / n_out
    x, idx = step * 0.5, np.empty(n_out, np.int64)
    for i in range(n_out):
        idx[i] = int(x)
        x += step
    return np.clip(idx, 0, n_in - 1)


@dataclass
class Item:
    """One dataset item before the GPU pipeline."""
    index: int
    line: str                       # the split line
    folder: str
    frame_index: int
    side: Optional[str]             # "l" / "r", None for a one-field line
    paths: List[str]                # one per frame id, in frame_idxs order
    draw: ItemDraw
    images: List = field(default_factory=list)    # opened PIL images (header read, not decoded)
    size: Tuple[int, int] = (0, 0)                # native (height, width)
    frames: List[np.ndarray] = field(default_factory=list)   # decoded (h, w, 3) uint8, unflipped

    def close(self):
        """Closes the image files still open."""
        for im in self.images:
            im.close()
        self.images = []


class MonoDataset:
    """mono_dataset.py:28-209 without the per-item PIL work (see the module docstring)."""

    def __init__(self, data_path, filenames, height, width, frame_idxs, num_scales, is_train=False,
                 img_ext=".jpg", seed: int = 0, load_depth: bool = False):
        self.data_path = data_path
        self.filenames = list(filenames)
        self.height = height
        self.width = width
        self.num_scales = num_scales
        self.frame_idxs = list(frame_idxs)
        self.is_train = is_train
        self.img_ext = img_ext
        self.seed = seed
        self.epoch = 0
        # the reference loads depth_gt whenever the first line has a scan; here only when
        # asked for too (it feeds the validation monitor alone)
        self.load_depth = bool(load_depth) and self.check_depth()

    def __len__(self):
        return len(self.filenames)

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def parse(self, index: int, epoch: Optional[int] = None) -> Item:
        """The split line of `index` (mono_dataset.py:143-161): paths, side and draws."""
        text = self.filenames[index]
        line = text.split()
        folder = line[0]
        frame_index = int(line[1]) if len(line) == 3 else 0
        side = line[2] if len(line) == 3 else None
        paths = []
        for i in self.frame_idxs:
            if i == "s":
                other_side = {"r": "l", "l": "r"}[side]
                paths.append(self.get_image_path(folder, frame_index, other_side))
            else:
                paths.append(self.get_image_path(folder, frame_index + i, side))
        rng = random.Random(item_seed(self.seed, self.epoch if epoch is None else epoch, index))
        return Item(index, text, folder, frame_index, side, paths, draw_item(rng, self.is_train))

    def open_item(self, index: int, epoch: Optional[int] = None) -> Item:
        """parse() plus the opened image files: sizes are known, nothing is decoded yet."""
        item = self.parse(index, epoch)
        try:
            for p in item.paths:
                try:
                    item.images.append(Image.open(p))
                except FileNotFoundError:
                    raise FileNotFoundError(f"split line {index} ({item.line!r}): no such image file {p}") from None
            sizes = {(im.size[1], im.size[0]) for im in item.images}
            if len(sizes) != 1:
                raise ValueError(f"split line {index} ({item.line!r}): its frames decode to different sizes "
                                 f"{sorted(sizes)}: {item.paths}")
        except BaseException:
            item.close()   # the files opened before the one that failed
            raise
        item.size = sizes.pop()
        return item

    @staticmethod
    def decode(image) -> np.ndarray:
        """pil_loader (mono_dataset.py:19-25): the file as (h, w, 3) uint8 RGB."""
        return np.asarray(image.convert("RGB"))

    def __getitem__(self, index: int) -> Item:
        item = self.open_item(index)
        try:
            item.frames = [self.decode(im) for im in item.images]
        finally:
            item.close()
        return item

    def get_image_path(self, folder, frame_index, side):
        raise NotImplementedError

    def check_depth(self):
        raise NotImplementedError

    def get_depth(self, folder, frame_index, side, do_flip):
        raise NotImplementedError

    def get_depths(self, items: Sequence[Item], device=None):
        """depth_gt of a batch as one (B, 375, 1242) float32 tensor on `device`: the
        items' host maps stacked, one upload."""
        import torch
        maps = np.stack([np.ascontiguousarray(self.get_depth(it.folder, it.frame_index, it.side, it.draw.do_flip),
                                              dtype=np.float32) for it in items])
        return torch.from_numpy(maps).to(device, non_blocking=True)


class KITTIDataset(MonoDataset):
    """kitti_dataset.py:18-55."""

    # normalised by the image size (kitti_dataset.py:29-32)
    K = np.array([[0.58, 0, 0.5, 0],
                  [0, 1.92, 0.5, 0],
                  [0, 0, 1, 0],
                  [0, 0, 0, 1]], dtype=np.float32)
    full_res_shape = (1242, 375)
    side_map = {"2": 2, "3": 3, "l": 2, "r": 3}

    def check_depth(self):
        line = self.filenames[0].split()
        scene_name = line[0]
        frame_index = int(line[1])
        velo_filename = os.path.join(self.data_path, scene_name,
                                     "velodyne_points/data/{:010d}.bin".format(int(frame_index)))
        return os.path.isfile(velo_filename)


class KITTIRAWDataset(KITTIDataset):
    """KITTI raw: ground truth from the velodyne scans (kitti_dataset.py:58-85)."""

    def get_image_path(self, folder, frame_index, side):
        f_str = "{:010d}{}".format(frame_index, self.img_ext)
        return os.path.join(self.data_path, folder, "image_0{}/data".format(self.side_map[side]), f_str)

    def get_depths(self, items: Sequence[Item], device=None):
        """depth_gt of a batch as one (B, 375, 1242) float32 device tensor.  The projection
        is the reference's (kitti_utils.generate_depth_maps): one call per camera in the
        batch, which reads each calibration folder once and shares a launch chain among
        the scans of one calibrated size.  Where that size is not 375 x 1242 the maps are
        resampled with PIL's NEAREST index rule, one gather per size; the reference's
        skimage resize(order=0) is not available to compare against."""
        import torch

        from .kitti_utils import generate_depth_maps
        W, H = self.full_res_shape
        out = None
        for cam in sorted({self.side_map[it.side] for it in items}):
            which = [b for b, it in enumerate(items) if self.side_map[it.side] == cam]
            frames = [(os.path.join(self.data_path, items[b].folder.split("/")[0]),
                       os.path.join(self.data_path, items[b].folder,
                                    "velodyne_points/data/{:010d}.bin".format(int(items[b].frame_index))))
                      for b in which]
            maps = generate_depth_maps(frames, cam, device=device)
            if out is None:
                out = torch.empty(len(items), H, W, dtype=torch.float32, device=maps[0].device)
            by_size = {}
            for b, m in zip(which, maps):
                by_size.setdefault(tuple(m.shape), []).append((b, m))
            for (h, w), group in by_size.items():
                stacked = torch.stack([m for _, m in group])
                if (h, w) != (H, W):
                    rows = torch.from_numpy(nearest_index(h, H)).to(stacked.device)
                    cols = torch.from_numpy(nearest_index(w, W)).to(stacked.device)
                    stacked = stacked[:, rows][:, :, cols]
                for j, (b, _) in enumerate(group):
                    out[b].copy_(torch.flip(stacked[j], [1]) if items[b].draw.do_flip else stacked[j])
        return out

    def get_depth(self, folder, frame_index, side, do_flip, device=None):
        """(375, 1242) float32 on the device: get_depths for one frame."""
        item = Item(-1, "", folder, int(frame_index), side, [], ItemDraw(bool(do_flip), False))
        return self.get_depths([item], device)[0]


class KITTIOdomDataset(KITTIDataset):
    """KITTI odometry sequences (kitti_dataset.py:88-101)."""

    def get_image_path(self, folder, frame_index, side):
        f_str = "{:06d}{}".format(frame_index, self.img_ext)
        return os.path.join(self.data_path, "sequences/{:02d}".format(int(folder)),
                            "image_{}".format(self.side_map[side]), f_str)


class KITTIDepthDataset(KITTIDataset):
    """KITTI with the updated ground-truth depth maps (kitti_dataset.py:104-134)."""

    def get_image_path(self, folder, frame_index, side):
        f_str = "{:010d}{}".format(frame_index, self.img_ext)
        return os.path.join(self.data_path, folder, "image_0{}/data".format(self.side_map[side]), f_str)

    def get_depth(self, folder, frame_index, side, do_flip, device=None):
        """(375, 1242) float32 on the host, as the reference (kitti_dataset.py:119-134)."""
        f_str = "{:010d}.png".format(frame_index)
        depth_path = os.path.join(self.data_path, folder,
                                  "proj_depth/groundtruth/image_0{}".format(self.side_map[side]), f_str)
        depth_gt = Image.open(depth_path)
        depth_gt = depth_gt.resize(self.full_res_shape, Image.NEAREST)
        depth_gt = np.array(depth_gt).astype(np.float32) / 256
        if do_flip:
            depth_gt = np.fliplr(depth_gt)
        return depth_gt


DATASETS = {"kitti": KITTIRAWDataset, "kitti_odom": KITTIOdomDataset, "kitti_depth": KITTIDepthDataset}
