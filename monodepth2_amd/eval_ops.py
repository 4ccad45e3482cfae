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

`benchmark_depth_maps(disp, ...)` is the `benchmark` split's export on the same prediction
(ABI `md2_depth_export16`, one launch): 16-bit maps of depth * 256 at 352 x 1216;
`write_benchmark_pngs` writes them as the reference's numbered PNGs.
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


def depth16_desc(batch: int, in_hw: Sequence[int], out_hw: Sequence[int] = (352, 1216), *, post_process: bool = False,
                 scale_factor: float = 5.4, clip_max: float = 80.0, quant: float = 256.0, min_depth: float = 0.1,
                 max_depth: float = 100.0) -> _lib.Depth16Desc:
    return _lib.Depth16Desc(batch, in_hw[0], in_hw[1], out_hw[0], out_hw[1],
                            _lib.DEPTH16_POST_PROCESS if post_process else 0, min_depth, max_depth, scale_factor,
                            clip_max, quant, 0)


def check_depth16(d: _lib.Depth16Desc):
    """Raises RuntimeError with the library's message for a desc md2_depth_export16 refuses."""
    _lib.check(_lib.lib().md2_depth_export16_check(ctypes.byref(d)), "md2_depth_export16_check")


def benchmark_depth_maps(disp: torch.Tensor, post_process_disp: Optional[torch.Tensor] = None,
                         out_hw: Sequence[int] = (352, 1216), scale_factor: float = 5.4, clip_max: float = 80.0,
                         quant: float = 256.0, min_depth: float = 0.1, max_depth: float = 100.0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The KITTI benchmark's 16-bit depth maps of `disp` (B,1,h,w) or (B,h,w), the raw
    sigmoid output, in one launch (csrc/eval.hip, `md2_depth_export16`): the export loop of
    evaluate_depth.py:148-163.  Per output pixel: disp_to_depth's scaled disparity,
    post-processed with `post_process_disp` (the output for the flipped images, not flipped
    back) if given, resized to `out_hw` with half-pixel bilinear weights in fp64, then
    (uint16)(min(max(scale_factor / r, 0), clip_max) * quant), truncated.  r == 0 gives
    clip_max * quant, a negative r gives 0, NaN gives 0 (this build's choice: the reference
    leaves them to numpy's undefined casts).

    Returns (B, OH, OW) on the device in torch.int16 storage that holds the uint16 bit
    patterns (a depth above 127.996 m at 256 counts per metre reads negative as int16);
    `.cpu().numpy().view(np.uint16)` is the image.  `out`: a (B, OH, OW) contiguous int16
    tensor on disp's device to write into (it may be a view at any 2-byte offset).
    Disparities that already went through disp_to_depth: min_depth=1, max_depth=inf.
    GPU only; the input checks are depth_metrics'.
    """
    if not torch.is_tensor(disp) or not disp.is_cuda:
        raise RuntimeError("benchmark_depth_maps is GPU only (HIP kernels, no CPU fallback)")
    if disp.dim() == 3:
        disp = disp.unsqueeze(1)
    if disp.dim() != 4 or disp.shape[1] != 1:
        raise ValueError(f"expected disp (B,1,h,w) or (B,h,w), got {tuple(disp.shape)}")
    if disp.dtype != torch.float32:
        raise ValueError("benchmark_depth_maps supports float32")
    disp = disp.detach().contiguous()
    flipped = None
    if post_process_disp is not None:
        flipped = post_process_disp.detach()
        if flipped.dim() == 3:
            flipped = flipped.unsqueeze(1)
        if flipped.shape != disp.shape or flipped.dtype != torch.float32 or flipped.device != disp.device:
            raise ValueError("post_process_disp must match disp in shape, dtype and device")
        flipped = flipped.contiguous()
    B, _, h, w = disp.shape
    OH, OW = int(out_hw[0]), int(out_hw[1])
    d = depth16_desc(B, (h, w), (OH, OW), post_process=flipped is not None, scale_factor=scale_factor,
                     clip_max=clip_max, quant=quant, min_depth=min_depth, max_depth=max_depth)
    check_depth16(d)   # before `out` is sized from it
    if out is None:
        out = torch.empty((B, OH, OW), dtype=torch.int16, device=disp.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.int16 or tuple(out.shape) != (B, OH, OW)
          or out.device != disp.device or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int16 tensor of shape {(B, OH, OW)} on {disp.device}")
    _lib.check(_lib.lib().md2_depth_export16(ctypes.byref(d), disp.data_ptr(),
                                             flipped.data_ptr() if flipped is not None else None, out.data_ptr(),
                                             _lib.stream(disp.device)), "md2_depth_export16")
    return out


def write_benchmark_pngs(maps, save_dir: str, start: int = 0, device_encode: bool = False):
    """`maps` (N, OH, OW), benchmark_depth_maps' int16 tensor or a uint16 / int16 array, as
    the files `{:010d}.png` of `save_dir`, numbered from `start`: 16-bit greyscale PNGs
    (Pillow mode I;16), what evaluate_depth.py:161-162 writes through cv2.  Returns the paths.
    device_encode: the int16 device tensor is filtered and deflated where it lies
    (png_ops.encode_png_batch) and only the compressed bytes come to the host:
    the same pixels in files of other bytes.  GPU only."""
    import os

    if device_encode:
        from . import png_ops
        if not torch.is_tensor(maps) or not maps.is_cuda:
            raise RuntimeError("write_benchmark_pngs(device_encode=True) is GPU only (HIP kernels, no CPU fallback)")
        if maps.dim() != 3 or maps.dtype != torch.int16:
            raise ValueError(f"maps must be (N, OH, OW) int16, got {tuple(maps.shape)} {maps.dtype}")
        files = png_ops.encode_png_batch(maps.contiguous(), kind=png_ops.KIND_GRAY16)
        os.makedirs(save_dir, exist_ok=True)
        paths = []
        for i, data in enumerate(files):
            path = os.path.join(save_dir, "{:010d}.png".format(start + i))
            with open(path, "wb") as f:
                f.write(data)
            paths.append(path)
        return paths
    from PIL import Image
    arr = maps.cpu().numpy() if torch.is_tensor(maps) else np.asarray(maps)
    if arr.ndim != 3 or arr.dtype not in (np.int16, np.uint16):
        raise ValueError(f"maps must be (N, OH, OW) int16 or uint16, got {arr.shape} {arr.dtype}")
    arr = np.ascontiguousarray(arr).view(np.uint16)
    os.makedirs(save_dir, exist_ok=True)
    paths = []
    for i, a in enumerate(arr):
        path = os.path.join(save_dir, "{:010d}.png".format(start + i))
        Image.fromarray(a).save(path)   # a uint16 array is mode I;16
        paths.append(path)
    return paths
