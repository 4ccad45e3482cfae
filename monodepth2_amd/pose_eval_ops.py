"""Absolute trajectory error of predicted poses on the device (csrc/traj.hip, `md2_pose_ate`).

`trajectory_ate(pred_poses, gt_global_poses, offsets, track_length)` takes the (N,4,4)
fp32 transforms of consecutive frame pairs (what the reference stores in poses.npy) and
the (M,3,4) fp64 KITTI global poses of one or several sequences and returns the
reference's per-snippet ATEs (evaluate_pose.py:104-125) with the mean and the population
standard deviation per sequence, every step in fp64, in three launches.  Nothing is read
back: the caller decides when to synchronise.  There is no CPU path: a CPU tensor is an
error.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple, Union

import torch

from . import _lib


def pose_ate_desc(sequences: int, total_frames: int, track_length: int = 5) -> _lib.PoseAteDesc:
    return _lib.PoseAteDesc(sequences, track_length, 0, 0, total_frames, 0)


def workspace_bytes(sequences: int, total_frames: int, track_length: int = 5) -> int:
    d = pose_ate_desc(sequences, total_frames, track_length)
    n = _lib.lib().md2_pose_ate_workspace_bytes(ctypes.byref(d))
    if n == 0:
        _lib.check(-1, "md2_pose_ate_workspace_bytes")
    return n


def check_offsets(offsets, total_frames: int, num_pred: int):
    """The contract the kernel cannot check without a synchronisation, on a host copy:
    0 = offsets[0] < ... < offsets[S] = total_frames, every sequence at least two frames,
    and one predicted transform per consecutive pair: num_pred = total_frames - S."""
    o = [int(v) for v in offsets]
    if len(o) < 2 or o[0] != 0 or o[-1] != total_frames or any(a > b for a, b in zip(o, o[1:])):
        raise ValueError(f"offsets must rise from 0 to the number of frames ({total_frames}), got {o[:8]}"
                         f"{' ...' if len(o) > 8 else ''}")
    if any(b - a < 2 for a, b in zip(o, o[1:])):
        raise ValueError(f"offsets: every sequence needs at least 2 frames, got {o[:8]}{' ...' if len(o) > 8 else ''}")
    if num_pred != total_frames - (len(o) - 1):
        raise ValueError(f"offsets: {total_frames} frames in {len(o) - 1} sequences need "
                         f"{total_frames - (len(o) - 1)} predicted transforms, got {num_pred}")


def trajectory_ate(pred_poses: torch.Tensor, gt_global_poses: Union[torch.Tensor, Sequence[torch.Tensor]],
                   offsets: Optional[torch.Tensor] = None, track_length: int = 5,
                   workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """pred_poses: (N, 4, 4) float32.  gt_global_poses: (M, 3, 4) float64 on the same
    device, with `offsets` (S + 1,) int64 (None: one sequence) — checked by `check_offsets`
    when it is a host tensor, the kernel's contract when it is on the device — or a list
    of S per-sequence (M_s, 3, 4) tensors with `offsets=None`, concatenated here.
    N = M - S.  workspace: a uint8 device tensor of at least `workspace_bytes(...)`, 256-byte
    aligned, to use instead of allocating one (its contents do not matter).  Returns
    (ates (N,), stats (S, 2): mean, std), float64 on the device of `pred_poses`."""
    if not torch.is_tensor(pred_poses) or not pred_poses.is_cuda:
        raise RuntimeError("trajectory_ate is GPU only (HIP kernels, no CPU fallback)")
    if pred_poses.dim() != 3 or tuple(pred_poses.shape[1:]) != (4, 4) or pred_poses.dtype != torch.float32:
        raise ValueError(f"pred_poses must be (N, 4, 4) float32, got {tuple(pred_poses.shape)} {pred_poses.dtype}")
    dev = pred_poses.device
    if isinstance(gt_global_poses, (list, tuple)):
        if offsets is not None:
            raise ValueError("offsets are built from a list of per-sequence poses: pass offsets=None")
        if not gt_global_poses:
            raise ValueError("no sequences")
        counts = [0]
        for g in gt_global_poses:
            if not torch.is_tensor(g) or g.dim() != 3 or tuple(g.shape[1:]) != (3, 4) or g.dtype != torch.float64:
                raise ValueError("every sequence's poses must be a (M, 3, 4) float64 tensor")
            counts.append(counts[-1] + g.shape[0])
        offsets = torch.tensor(counts, dtype=torch.int64)
        gt_global_poses = torch.cat(list(gt_global_poses), 0)
    gt = gt_global_poses
    if not torch.is_tensor(gt) or gt.dim() != 3 or tuple(gt.shape[1:]) != (3, 4) or gt.dtype != torch.float64:
        raise ValueError("gt_global_poses must be (M, 3, 4) float64" +
                         (f", got {tuple(gt.shape)} {gt.dtype}" if torch.is_tensor(gt) else ""))
    if not gt.is_cuda:
        raise RuntimeError("trajectory_ate is GPU only (HIP kernels, no CPU fallback)")
    N, M = pred_poses.shape[0], gt.shape[0]
    if offsets is None:
        offsets = torch.tensor([0, M], dtype=torch.int64)
    if not torch.is_tensor(offsets) or offsets.dim() != 1 or offsets.shape[0] < 2 or offsets.dtype != torch.int64:
        raise ValueError("offsets must be (S + 1,) int64")
    S = offsets.shape[0] - 1
    if not offsets.is_cuda:
        check_offsets(offsets.tolist(), M, N)
        offsets = offsets.to(dev, non_blocking=True)
    elif N != M - S:
        raise ValueError(f"{M} frames in {S} sequences need {M - S} predicted transforms, got {N}")
    if gt.device != dev or offsets.device != dev:
        raise ValueError("pred_poses, gt_global_poses and offsets must be on the same device")
    pred, gt, offsets = pred_poses.detach().contiguous(), gt.detach().contiguous(), offsets.contiguous()
    d = pose_ate_desc(S, M, int(track_length))
    L = _lib.lib()
    nbytes = L.md2_pose_ate_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        _lib.check(-1, "md2_pose_ate_workspace_bytes")   # MD2_ERR_ARG: md2_last_error says why
    if workspace is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        ws = workspace
        if ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < nbytes:
            raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}")
    ates = torch.empty(N, dtype=torch.float64, device=dev)
    stats = torch.empty((S, 2), dtype=torch.float64, device=dev)
    _lib.check(L.md2_pose_ate(ctypes.byref(d), pred.data_ptr(), gt.data_ptr(), offsets.data_ptr(), ates.data_ptr(),
                              stats.data_ptr(), ws.data_ptr(), _lib.stream(dev)), "md2_pose_ate")
    return ates, stats
