"""Depth metrics on the device: the seven Eigen numbers of predicted disparities against
sparse ground truth in one chain of HIP launches (csrc/eval.hip, ABI `md2_depth_eval`).

`depth_metrics(disp, gt, ...)` takes the network's sigmoid output (B,1,h,w) and ground
truth (B,GH,GW) and returns a (P,10) device tensor — abs_rel, sq_rel, rmse, rmse_log, a1,
a2, a3, the median ratio applied, the valid-pixel count, 0 — for P = B populations (or 1
with `pool_batch`).  Nothing is read back: the caller decides when to synchronise.

Two formulations of the reference are selectable:

* ``mode="evaluate"`` — evaluate_depth.py:181-214: the scaled disparity is resized to the
  ground-truth map and inverted, masked, median-scaled per image with `np.median`'s
  convention, clamped to [1e-3, 80].
* ``mode="monitor"`` — Trainer.compute_depth_losses (trainer.py:498-526): the depth is
  resized and clamped, masked with gt > 0, median-scaled over the whole batch with
  `torch.median`'s convention (the lower middle element), clamped again.

The resize is half-pixel bilinear (F.interpolate(align_corners=False)); cv2.resize of the
reference's evaluate_depth.py is the same formula, bit parity with it is not measured.
There is no CPU path: a CPU tensor is an error.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

METRIC_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
RATIO, COUNT = 7, 8   # columns of the result after the seven metrics
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0   # evaluate_depth.py:62-63


def eigen_crop(gt_height: int, gt_width: int) -> Tuple[int, int, int, int]:
    """(y0, y1, x0, x1) of evaluate_depth.py:193-194; 375 x 1242 gives the trainer's
    153:371, 44:1197 (trainer.py:510)."""
    c = np.array([0.40810811 * gt_height, 0.99189189 * gt_height,
                  0.03594771 * gt_width, 0.96405229 * gt_width]).astype(np.int32)
    return int(c[0]), int(c[1]), int(c[2]), int(c[3])


def eval_desc(batch: int, height: int, width: int, gt_height: int, gt_width: int, *, mode: str = "evaluate",
              post_process: bool = False, median_scaling: bool = True, scale_factor: float = 1.0,
              crop: Union[str, None, Sequence[int]] = "eigen", gt_range: Optional[bool] = None,
              pool_batch: Optional[bool] = None, median_lower: Optional[bool] = None,
              min_depth: float = 0.1, max_depth: float = 100.0, eval_min: float = MIN_DEPTH,
              eval_max: float = MAX_DEPTH) -> _lib.EvalDesc:
    if mode not in ("evaluate", "monitor"):
        raise ValueError(f"mode must be 'evaluate' or 'monitor', got {mode!r}")
    monitor = mode == "monitor"
    if isinstance(crop, str):
        if crop != "eigen":
            raise ValueError(f"crop must be 'eigen', None or (y0, y1, x0, x1), got {crop!r}")
        rect = eigen_crop(gt_height, gt_width)
    elif crop is None:
        rect = (0, gt_height, 0, gt_width)
    else:
        rect = tuple(int(v) for v in crop)
        if len(rect) != 4:
            raise ValueError("crop must be (y0, y1, x0, x1)")
    if gt_range is None:   # evaluate_depth.py:190-200: the range mask goes with the Eigen crop
        gt_range = (not monitor) and isinstance(crop, str)
    pool_batch = monitor if pool_batch is None else pool_batch
    median_lower = monitor if median_lower is None else median_lower
    flags = ((_lib.EVAL_POST_PROCESS if post_process else 0) | (_lib.EVAL_RESIZE_DEPTH if monitor else 0)
             | (_lib.EVAL_GT_RANGE if gt_range else 0) | (_lib.EVAL_MEDIAN_SCALE if median_scaling else 0)
             | (_lib.EVAL_MEDIAN_LOWER if median_lower else 0) | (_lib.EVAL_POOL_BATCH if pool_batch else 0))
    return _lib.EvalDesc(batch, height, width, gt_height, gt_width, rect[0], rect[1], rect[2], rect[3], flags,
                         min_depth, max_depth, eval_min, eval_max, scale_factor)


def depth_metrics(disp: torch.Tensor, gt: torch.Tensor, *, mode: str = "evaluate",
                  post_process_disp: Optional[torch.Tensor] = None, median_scaling: bool = True,
                  scale_factor: float = 1.0, crop: Union[str, None, Sequence[int]] = "eigen",
                  gt_range: Optional[bool] = None, pool_batch: Optional[bool] = None,
                  median_lower: Optional[bool] = None, min_depth: float = 0.1, max_depth: float = 100.0,
                  eval_min: float = MIN_DEPTH, eval_max: float = MAX_DEPTH, return_pred: bool = False):
    """The metrics of `disp` (B,1,h,w) or (B,h,w), the raw sigmoid output, against `gt`
    (B,GH,GW) or (B,1,GH,GW) -> (P,10) float32 on the device.

    post_process_disp: the network's output for the horizontally flipped images (as it
    comes out, not flipped back): the reference's batch_post_process_disparity is applied.
    crop: "eigen" (the Eigen crop of the ground-truth size), None, or (y0, y1, x0, x1).
    gt_range / pool_batch / median_lower default to what `mode` does in the reference.
    return_pred: also return the (B,GH,GW) fp32 prediction before the median scaling and
    its validity mask (the kernel's own planes; tests check the medians against them).
    """
    if not disp.is_cuda:
        raise RuntimeError("depth_metrics is GPU only (HIP kernels, no CPU fallback)")
    if disp.dim() == 3:
        disp = disp.unsqueeze(1)
    if gt.dim() == 4:
        gt = gt[:, 0]
    if disp.dim() != 4 or disp.shape[1] != 1 or gt.dim() != 3 or gt.shape[0] != disp.shape[0]:
        raise ValueError(f"expected disp (B,1,h,w) and gt (B,GH,GW), got {tuple(disp.shape)} / {tuple(gt.shape)}")
    if disp.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError("depth_metrics supports float32")
    if gt.device != disp.device:
        raise ValueError("disp and gt must be on the same device")
    disp, gt = disp.detach().contiguous(), gt.detach().contiguous()
    flipped = None
    if post_process_disp is not None:
        flipped = post_process_disp.detach()
        if flipped.dim() == 3:
            flipped = flipped.unsqueeze(1)
        if flipped.shape != disp.shape or flipped.dtype != torch.float32 or flipped.device != disp.device:
            raise ValueError("post_process_disp must match disp in shape, dtype and device")
        flipped = flipped.contiguous()
    B, _, h, w = disp.shape
    GH, GW = gt.shape[1:]
    d = eval_desc(B, h, w, GH, GW, mode=mode, post_process=flipped is not None, median_scaling=median_scaling,
                  scale_factor=scale_factor, crop=crop, gt_range=gt_range, pool_batch=pool_batch,
                  median_lower=median_lower, min_depth=min_depth, max_depth=max_depth, eval_min=eval_min,
                  eval_max=eval_max)
    L = _lib.lib()
    nbytes = L.md2_depth_eval_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        _lib.check(-1, "md2_depth_eval_workspace_bytes")   # MD2_ERR_ARG: md2_last_error says why
    ws = torch.empty(nbytes, dtype=torch.uint8, device=disp.device)
    P = 1 if d.flags & _lib.EVAL_POOL_BATCH else B
    out = torch.empty((P, _lib.EVAL_OUT), dtype=torch.float32, device=disp.device)
    _lib.check(L.md2_depth_eval(ctypes.byref(d), disp.data_ptr(), flipped.data_ptr() if flipped is not None else None,
                                gt.data_ptr(), out.data_ptr(), ws.data_ptr(), _lib.stream(disp.device)),
               "md2_depth_eval")
    if not return_pred:
        return out
    keys = ws[:4 * B * GH * GW].view(torch.int32).view(B, GH, GW)
    return out, keys.view(torch.float32), keys != -1
