"""A batch of depth predictions as a point cloud on the device (csrc/points.hip,
`md2_depth_points`).

`depth_to_points(map, rgb, inv_K, T)` is the reference's `disp_to_depth` (layers.py:16-25)
and `BackprojectDepth` (layers.py:139-168) per pixel in fp32 at the image's own size, with
the pixels that are off the stride grid, outside [near, far] or not finite dropped, the
survivors compacted in (image, row, column) order and packed as the 15-byte vertex records
of a binary PLY file: the device buffer is the file's body.  Nothing is read back: the
caller reads `offsets[-1]` when it wants the count, and slices.  There is no CPU path: a CPU
tensor is an error.  `write_ply` is host-only.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib

RECORD_BYTES = _lib.POINTS_RECORD_BYTES
# one vertex record as numpy reads it back: np.frombuffer(body, VERTEX_DTYPE)
VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
assert VERTEX_DTYPE.itemsize == RECORD_BYTES


def points_desc(batch: int, height: int, width: int, *, depth_input: bool = False, world: bool = False,
                min_depth: float = 0.1, max_depth: float = 100.0, depth_scale: float = 1.0, near: float = 1e-3,
                far: float = 80.0, stride: int = 1) -> _lib.PointsDesc:
    """disp_a and disp_b are formed in double and rounded once, as torch forms the Python
    scalars of disp_to_depth: max_disp - min_disp, and min_disp."""
    if depth_input:
        disp_a = disp_b = 0.0
    else:
        disp_a, disp_b = 1 / min_depth - 1 / max_depth, 1 / max_depth
    flags = (_lib.POINTS_DEPTH_INPUT if depth_input else 0) | (_lib.POINTS_WORLD if world else 0)
    return _lib.PointsDesc(batch, height, width, stride, disp_a, disp_b, depth_scale, near, far, flags, (0, 0))


def capacity(batch: int, height: int, width: int, stride: int = 1) -> int:
    """The records a call can produce: every pixel of the stride grid."""
    return batch * (-(-height // stride)) * (-(-width // stride))


def workspace_bytes(batch: int, height: int, width: int, **kw) -> int:
    d = points_desc(batch, height, width, **kw)
    n = _lib.lib().md2_depth_points_workspace_bytes(ctypes.byref(d))
    if n == 0:
        _lib.check(-1, "md2_depth_points_workspace_bytes")
    return n


def depth_to_points(map: torch.Tensor, rgb: torch.Tensor, inv_K: torch.Tensor, T: Optional[torch.Tensor] = None, *,
                    depth_input: bool = False, min_depth: float = 0.1, max_depth: float = 100.0,
                    depth_scale: float = 1.0, near: float = 1e-3, far: float = 80.0, stride: int = 1,
                    workspace: Optional[torch.Tensor] = None):
    """map: (B, H, W) or (B, 1, H, W) float32 on the device, the network's sigmoid disparity
    at the image's size (or depth with `depth_input`); rgb: (B, H, W, 3) uint8; inv_K:
    (B, 4, 4) float32; T: (B, 4, 4) float32 camera-to-world, or None for the camera frame.
    workspace: a uint8 device tensor of at least `workspace_bytes(...)`, 256-byte aligned, to
    use instead of allocating one.  Returns (vertices, offsets): a uint8 tensor of
    15 * capacity bytes whose first 15 * offsets[-1] bytes are the records, and the (B + 1)
    record offsets of the images (int32 storage of the kernel's uint32, below 2^31)."""
    for name, t in (("map", map), ("rgb", rgb), ("inv_K", inv_K)) + ((("T", T),) if T is not None else ()):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"depth_to_points is GPU only (HIP kernels, no CPU fallback): {name} is not on a GPU")
    if map.dim() == 4 and map.shape[1] == 1:
        map = map[:, 0]
    if map.dim() != 3 or map.dtype != torch.float32:
        raise ValueError(f"map must be (B, H, W) or (B, 1, H, W) float32, got {tuple(map.shape)} {map.dtype}")
    B, H, W = map.shape
    if tuple(rgb.shape) != (B, H, W, 3) or rgb.dtype != torch.uint8:
        raise ValueError(f"rgb must be ({B}, {H}, {W}, 3) uint8, got {tuple(rgb.shape)} {rgb.dtype}")
    if tuple(inv_K.shape) != (B, 4, 4) or inv_K.dtype != torch.float32:
        raise ValueError(f"inv_K must be ({B}, 4, 4) float32, got {tuple(inv_K.shape)} {inv_K.dtype}")
    if T is not None and (tuple(T.shape) != (B, 4, 4) or T.dtype != torch.float32):
        raise ValueError(f"T must be ({B}, 4, 4) float32, got {tuple(T.shape)} {T.dtype}")
    if int(stride) != stride:
        raise ValueError(f"stride must be an integer, got {stride!r}")
    dev = map.device
    if any(t.device != dev for t in (rgb, inv_K) + ((T,) if T is not None else ())):
        raise ValueError(f"map, rgb, inv_K and T must be on one device ({dev})")
    map, rgb, inv_K = map.detach().contiguous(), rgb.contiguous(), inv_K.detach().contiguous()
    T = T.detach().contiguous() if T is not None else None
    d = points_desc(B, H, W, depth_input=depth_input, world=T is not None, min_depth=min_depth, max_depth=max_depth,
                    depth_scale=depth_scale, near=near, far=far, stride=int(stride))
    L = _lib.lib()
    nbytes = L.md2_depth_points_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        _lib.check(-1, "md2_depth_points_workspace_bytes")   # MD2_ERR_ARG: md2_last_error says why
    if workspace is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        ws = workspace
        if ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < nbytes:
            raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}")
    cap = capacity(B, H, W, int(stride))
    vertices = torch.empty(cap * RECORD_BYTES, dtype=torch.uint8, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
    _lib.check(L.md2_depth_points(ctypes.byref(d), map.data_ptr(), rgb.data_ptr(), inv_K.data_ptr(),
                                  T.data_ptr() if T is not None else None, vertices.data_ptr(), cap,
                                  offsets.data_ptr(), ws.data_ptr(), _lib.stream(dev)), "md2_depth_points")
    return vertices, offsets


def ply_header(count: int) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\nelement vertex {:d}\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
            ).format(int(count)).encode("ascii")


def write_ply(path, vertices_bytes, count: int) -> None:
    """A binary little-endian PLY file of `count` vertices: the header, then the first
    15 * count bytes of `vertices_bytes` (a uint8 numpy array, a CPU uint8 tensor or a bytes
    object: the operator's buffer after a copy to the host) as they are."""
    if torch.is_tensor(vertices_bytes):
        if vertices_bytes.is_cuda:
            raise ValueError("write_ply is host-only: copy the vertices to the CPU first")
        vertices_bytes = vertices_bytes.numpy()
    body = np.frombuffer(vertices_bytes, np.uint8) if isinstance(vertices_bytes, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(vertices_bytes)
    if body.dtype != np.uint8:
        raise ValueError(f"vertices_bytes must be uint8, got {body.dtype}")
    body = body.reshape(-1)
    count = int(count)
    if count < 0 or body.size < count * RECORD_BYTES:
        raise ValueError(f"{count} records need {count * RECORD_BYTES} bytes, got {body.size}")
    with open(path, "wb") as f:
        f.write(ply_header(count))
        f.write(body[:count * RECORD_BYTES].tobytes())


def read_ply(path):
    """The vertices of a file `write_ply` wrote, as a VERTEX_DTYPE array (for tests and
    quick looks; not a general PLY reader)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    count = None
    for line in data[:end].decode("ascii").split("\n"):
        if line.startswith("element vertex "):
            count = int(line.split()[2])
    if count is None or data[:end] != ply_header(count):
        raise ValueError(f"{path}: not a header write_ply writes")
    if len(data) - end != count * RECORD_BYTES:
        raise ValueError(f"{path}: {count} vertices need {count * RECORD_BYTES} body bytes, found {len(data) - end}")
    return np.frombuffer(data, VERTEX_DTYPE, count, end)
