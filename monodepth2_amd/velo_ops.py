"""Velodyne scans to sparse depth maps on the device (csrc/velo.hip, `md2_velo_project`).

`project_velodyne(points, offsets, P, height, width)` takes the concatenated fp32 points
of B scans, their row offsets and one fp64 3x4 projection per scan, and returns the
(B, height, width) fp32 maps the reference's kitti_utils.generate_depth_map
(kitti_utils.py:46-98) produces per frame — last point per pixel first, then the minimum
of every duplicate group under the reference's own `sub2ind` key, which columns 0 and
W-1 of neighbouring rows share — in three launches.  Nothing is read back: the caller
decides when to synchronise.  There is no CPU path: a CPU tensor is an error.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Union

import torch

from . import _lib


def velo_desc(batch: int, height: int, width: int, total_points: int, vel_depth: bool = False) -> _lib.VeloDesc:
    return _lib.VeloDesc(batch, height, width, _lib.VELO_VEL_DEPTH if vel_depth else 0, total_points)


def workspace_bytes(batch: int, height: int, width: int, total_points: int) -> int:
    d = velo_desc(batch, height, width, total_points)
    n = _lib.lib().md2_velo_project_workspace_bytes(ctypes.byref(d))
    if n == 0:
        _lib.check(-1, "md2_velo_project_workspace_bytes")
    return n


def check_offsets(offsets, total_points: int):
    """The contract the kernel cannot check without a synchronisation, on a host copy:
    0 = offsets[0] <= ... <= offsets[B] = total_points."""
    o = [int(v) for v in offsets]
    if not o or o[0] != 0 or o[-1] != total_points or any(a > b for a, b in zip(o, o[1:])):
        raise ValueError(f"offsets must rise from 0 to the number of points ({total_points}), got {o[:8]}"
                         f"{' ...' if len(o) > 8 else ''}")


def project_velodyne(points: Union[torch.Tensor, Sequence[torch.Tensor]], offsets: Optional[torch.Tensor],
                     P: torch.Tensor, height: int, width: int, vel_depth: bool = False,
                     workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """points: (total, 4) float32 rows x, y, z, reflectance of all frames, with `offsets`
    (B + 1,) int64 on the same device (rising from 0 to total: checked only when it is a
    host tensor, the kernel's contract otherwise) — or a list of B per-frame (n_b, 4)
    tensors with `offsets=None`, concatenated here.  P: (B, 3, 4) float64 (or (3, 4) for
    one frame).  workspace: a uint8 device tensor of at least `workspace_bytes(...)` to use
    instead of allocating one (its contents do not matter).  Returns (B, height, width)
    float32 on the device of `points`."""
    if isinstance(points, (list, tuple)):
        if offsets is not None:
            raise ValueError("offsets are built from a list of per-frame points: pass offsets=None")
        if not points:
            raise ValueError("no frames")
        for p in points:
            if not torch.is_tensor(p) or p.dim() != 2 or p.shape[1] != 4:
                raise ValueError("every frame's points must be a (n, 4) tensor")
        if not points[0].is_cuda:
            raise RuntimeError("project_velodyne is GPU only (HIP kernels, no CPU fallback)")
        counts = [0]
        for p in points:
            counts.append(counts[-1] + p.shape[0])
        offsets = torch.tensor(counts, dtype=torch.int64).to(points[0].device, non_blocking=True)
        points = torch.cat(list(points), 0)
    if not torch.is_tensor(points) or not points.is_cuda:
        raise RuntimeError("project_velodyne is GPU only (HIP kernels, no CPU fallback)")
    if points.dim() != 2 or points.shape[1] != 4 or points.dtype != torch.float32:
        raise ValueError(f"points must be (total, 4) float32, got {tuple(points.shape)} {points.dtype}")
    if P.dim() == 2:
        P = P.unsqueeze(0)
    if P.dim() != 3 or tuple(P.shape[1:]) != (3, 4) or P.dtype != torch.float64:
        raise ValueError(f"P must be (B, 3, 4) float64, got {tuple(P.shape)} {P.dtype}")
    B, total = P.shape[0], points.shape[0]
    if not torch.is_tensor(offsets) or offsets.dim() != 1 or offsets.shape[0] != B + 1 or offsets.dtype != torch.int64:
        raise ValueError(f"offsets must be ({B + 1},) int64")
    if not offsets.is_cuda:
        check_offsets(offsets.tolist(), total)
        offsets = offsets.to(points.device, non_blocking=True)
    if P.device != points.device or offsets.device != points.device:
        raise ValueError("points, offsets and P must be on the same device")
    depth = torch.empty((B, int(height), int(width)), dtype=torch.float32, device=points.device)
    if total == 0:   # the C entry refuses an empty operand; all maps are empty
        return depth.zero_()
    points, offsets, P = points.detach().contiguous(), offsets.contiguous(), P.detach().contiguous()
    d = velo_desc(B, int(height), int(width), total, vel_depth)
    L = _lib.lib()
    nbytes = L.md2_velo_project_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        _lib.check(-1, "md2_velo_project_workspace_bytes")   # MD2_ERR_ARG: md2_last_error says why
    if workspace is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    else:
        ws = workspace
        if ws.dtype != torch.uint8 or ws.device != points.device or not ws.is_contiguous() or ws.numel() < nbytes:
            raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {points.device}")
    _lib.check(L.md2_velo_project(ctypes.byref(d), points.data_ptr(), offsets.data_ptr(), P.data_ptr(),
                                  depth.data_ptr(), ws.data_ptr(), _lib.stream(points.device)),
               "md2_velo_project")
    return depth
