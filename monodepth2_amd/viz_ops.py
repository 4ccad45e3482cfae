"""A batch of disparities as the reference's colour pictures on the device (csrc/viz.hip,
`md2_disp_colorize`).

`colorize_disparity(disp, size, percentile)` is the tail of the reference's test_simple.py
(136-155): the bilinear resize to the original image size, np.percentile(., 95) and .min()
per image, matplotlib's Normalize and `magma`, uint8 — one chain of launches for the whole
batch instead of numpy and matplotlib per image on the host.  Nothing is read back: the
caller decides when to synchronise.  There is no CPU path: a CPU tensor is an error.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib


def viz_desc(batch: int, in_hw: Sequence[int], out_hw: Sequence[int], percentile: int = 95) -> _lib.VizDesc:
    return _lib.VizDesc(batch, in_hw[0], in_hw[1], out_hw[0], out_hw[1], percentile, 0, 0)


def workspace_bytes(batch: int, in_hw: Sequence[int], out_hw: Sequence[int], percentile: int = 95) -> int:
    d = viz_desc(batch, in_hw, out_hw, percentile)
    n = _lib.lib().md2_disp_colorize_workspace_bytes(ctypes.byref(d))
    if n == 0:
        _lib.check(-1, "md2_disp_colorize_workspace_bytes")
    return n


def colorize_disparity(disp: torch.Tensor, size: Optional[Sequence[int]] = None, percentile: int = 95,
                       return_resized: bool = False, return_stats: bool = False,
                       workspace: Optional[torch.Tensor] = None):
    """disp: (B, 1, h, w) or (B, h, w) float32 on the device.  size: (H, W) of the pictures
    (None: h, w).  percentile: an integer 0..100, the reference's 95.  workspace: a uint8
    device tensor of at least `workspace_bytes(...)`, 256-byte aligned, to use instead of
    allocating one (its contents do not matter).  Returns rgb (B, H, W, 3) uint8 on the
    device of `disp`; with return_resized / return_stats a tuple that also holds the resized
    maps (B, H, W) float32 and / or (B, 2) float32 vmin, vmax per image, in that order."""
    if not torch.is_tensor(disp) or not disp.is_cuda:
        raise RuntimeError("colorize_disparity is GPU only (HIP kernels, no CPU fallback)")
    if disp.dim() == 4 and disp.shape[1] == 1:
        disp = disp[:, 0]
    if disp.dim() != 3 or disp.dtype != torch.float32:
        raise ValueError(f"disp must be (B, 1, h, w) or (B, h, w) float32, got {tuple(disp.shape)} {disp.dtype}")
    if int(percentile) != percentile:
        raise ValueError(f"percentile must be an integer 0..100, got {percentile!r}")
    dev = disp.device
    disp = disp.detach().contiguous()
    B, h, w = disp.shape
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    d = viz_desc(B, (h, w), (H, W), int(percentile))
    L = _lib.lib()
    nbytes = L.md2_disp_colorize_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        _lib.check(-1, "md2_disp_colorize_workspace_bytes")   # MD2_ERR_ARG: md2_last_error says why
    if workspace is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        ws = workspace
        if ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < nbytes:
            raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}")
    rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    resized = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_resized else None
    stats = torch.empty((B, 2), dtype=torch.float32, device=dev) if return_stats else None
    _lib.check(L.md2_disp_colorize(ctypes.byref(d), disp.data_ptr(), rgb.data_ptr(),
                                   resized.data_ptr() if resized is not None else None,
                                   stats.data_ptr() if stats is not None else None,
                                   ws.data_ptr(), _lib.stream(dev)), "md2_disp_colorize")
    out = (rgb,) + ((resized,) if return_resized else ()) + ((stats,) if return_stats else ())
    return out if len(out) > 1 else rgb
