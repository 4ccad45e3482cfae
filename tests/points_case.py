"""The yardstick of the point-cloud tests: a numpy restatement of md2_depth_points
(include/md2hot.h; the reference's disp_to_depth, layers.py:16-25, and BackprojectDepth,
layers.py:139-168) in the kernel's written order — every product and sum one separately
rounded fp32 operation on numpy arrays, the filter, the compaction in np.nonzero order, the
15-byte records as a structured dtype — no torch.  The case inputs and the loaders of
tests/golden/points/points.npz are here too; tests/golden/points/make_points_golden.py
measures the restatement against the reference's own layers before it records the golden.
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points", "points.npz")
F32 = np.float32
VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
assert VERTEX.itemsize == 15

KITTI_K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=F32)


# ---- the restatement ---------------------------------------------------------------------

def disp_scalars(min_depth=0.1, max_depth=100.0):
    """disp_a, disp_b: formed in double, rounded once (torch's Python scalars)."""
    return F32(1 / min_depth - 1 / max_depth), F32(1 / max_depth)


def depth_np(m, depth_input=False, min_depth=0.1, max_depth=100.0):
    """Steps 1-2: (B,H,W) fp32 map -> depth."""
    m = np.ascontiguousarray(m, dtype=F32)
    if depth_input:
        return m
    a, b = disp_scalars(min_depth, max_depth)
    with np.errstate(all="ignore"):
        sd = (b + (a * m).astype(F32)).astype(F32)
        depth = (F32(1) / sd).astype(F32)
    assert depth.dtype == F32
    return depth


def camera_points_np(depth, inv_K, depth_scale=1.0):
    """Steps 3-5: z (B,H,W) and P (B,3,H,W), fp32 throughout."""
    B, H, W = depth.shape
    k = np.ascontiguousarray(inv_K, dtype=F32)
    x = np.arange(W, dtype=np.int64).astype(F32)[None, None, :]
    y = np.arange(H, dtype=np.int64).astype(F32)[None, :, None]
    with np.errstate(all="ignore"):
        z = (F32(depth_scale) * depth).astype(F32)
        P = np.empty((B, 3, H, W), F32)
        for i in range(3):
            k0, k1, k2 = (k[:, i, j][:, None, None] for j in range(3))
            r = (((k0 * x).astype(F32) + (k1 * y).astype(F32)).astype(F32) + k2).astype(F32)
            P[:, i] = (z * r).astype(F32)
    return z, P


def world_points_np(P, T):
    """Step 6: Q_i = ((t_i0 P_0 + t_i1 P_1) + t_i2 P_2) + t_i3."""
    t = np.ascontiguousarray(T, dtype=F32)
    Q = np.empty_like(P)
    with np.errstate(all="ignore"):
        for i in range(3):
            t0, t1, t2, t3 = (t[:, i, j][:, None, None] for j in range(4))
            s = ((t0 * P[:, 0]).astype(F32) + (t1 * P[:, 1]).astype(F32)).astype(F32)
            s = (s + (t2 * P[:, 2]).astype(F32)).astype(F32)
            Q[:, i] = (s + t3).astype(F32)
    return Q


def points_np(m, rgb, inv_K, T=None, depth_input=False, min_depth=0.1, max_depth=100.0, depth_scale=1.0,
              near=1e-3, far=80.0, stride=1):
    """The whole operator: (records (N,) VERTEX, offsets (B+1,) uint32, keep (B,H,W) bool,
    stored coordinates (B,3,H,W) fp32)."""
    m = np.ascontiguousarray(m, dtype=F32)
    if m.ndim == 4:
        m = m[:, 0]
    B, H, W = m.shape
    depth = depth_np(m, depth_input, min_depth, max_depth)
    z, P = camera_points_np(depth, inv_K, depth_scale)
    out = world_points_np(P, T) if T is not None else P
    with np.errstate(invalid="ignore"):
        keep = (z >= F32(near)) & (z <= F32(far)) & np.isfinite(out).all(axis=1)
    grid = np.zeros((H, W), bool)
    grid[::stride, ::stride] = True
    keep &= grid[None]
    b, y, x = np.nonzero(keep)                      # (image, row, column) order
    rec = np.empty(b.size, VERTEX)
    rec["x"], rec["y"], rec["z"] = out[b, 0, y, x], out[b, 1, y, x], out[b, 2, y, x]
    rec["red"], rec["green"], rec["blue"] = (rgb[b, y, x, c] for c in range(3))
    offsets = np.zeros(B + 1, np.uint32)
    offsets[1:] = np.cumsum(keep.reshape(B, -1).sum(1))
    return rec, offsets, keep, out


def reproject_np(rec, K):
    """Pixel coordinates of camera-frame records under the (4,4) K, in fp64."""
    P = np.stack([rec["x"], rec["y"], rec["z"]]).astype(np.float64)
    q = K[:3, :3].astype(np.float64) @ P
    return q[0] / q[2], q[1] / q[2]


# ---- cases -------------------------------------------------------------------------------

def intrinsics(H, W, B=1, K=KITTI_K):
    """(K, inv_K) of an image size as mono_dataset.py builds them, (B,4,4) fp32 each."""
    K = K.copy()
    K[0, :] *= W
    K[1, :] *= H
    inv_K = np.linalg.pinv(K)
    return np.repeat(K[None], B, 0), np.repeat(inv_K[None].astype(F32), B, 0)


def colours(B, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (B, H, W, 3)).astype(np.uint8)


def rigid(B, seed, reach=300.0):
    """Random rotations (QR of a normal matrix, det +1) and translations of hundreds of metres."""
    rng = np.random.RandomState(seed)
    T = np.zeros((B, 4, 4), np.float64)
    for b in range(B):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        T[b, :3, :3] = q
        T[b, :3, 3] = rng.uniform(-reach, reach, 3)
        T[b, 3, 3] = 1
    return T.astype(F32)


def golden_cases():
    """name -> (disp (B,H,W) fp32 in (0,1), inv_K, K): what the golden records the reference
    on.  Uniform random disparities, KITTI intrinsics."""
    c = {}
    for (B, H, W), seed in (((1, 5, 7), 1), ((3, 37, 50), 2), ((1, 64, 128), 3)):
        disp = np.random.RandomState(seed).uniform(0.0, 1.0, (B, H, W)).astype(F32)
        K, inv_K = intrinsics(H, W, B)
        c["g_%dx%dx%d" % (B, H, W)] = (disp, inv_K, K)
    return c


def ulp_up(v):
    return np.nextafter(F32(v), F32(np.inf))


def ulp_down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def kernel_cases():
    """name -> dict(map, rgb, inv_K, T or None, kw): the smallest shapes at which the kernel
    can go wrong.  A block takes 1024 candidates in four passes of 256 (four waves of 64).
    Random disparities with near = 0.15 lose about a third of their pixels (depth is
    1 / (0.01 + 9.99 d)), so ranks and block counts are irregular."""
    c = {}

    def add(name, m, seed, T=None, **kw):
        m = np.ascontiguousarray(m, dtype=F32)
        B, H, W = m.shape
        c[name] = dict(map=m, rgb=colours(B, H, W, seed), inv_K=intrinsics(H, W, B)[1], T=T, kw=kw)

    def disp(B, H, W, seed):
        return np.random.RandomState(seed).uniform(0.0, 1.0, (B, H, W)).astype(F32)

    add("1x1x1_kept", np.full((1, 1, 1), 0.5), 1)
    add("1x1x1_dropped", np.zeros((1, 1, 1)), 2)                      # depth 100 > far
    add("1x3x5", disp(1, 3, 5, 3), 3, near=0.15)
    add("row_65", disp(1, 1, 65, 4), 4, near=0.15)                    # a wave and one
    add("row_257", disp(1, 1, 257, 5), 5, near=0.15)                  # a pass and one
    add("row_1025", disp(1, 1, 1025, 6), 6, near=0.15)                # a block's candidates and one
    add("col_1025", disp(1, 1025, 1, 7), 7, near=0.15)
    # three differently built images: a checkerboard of random values against out-of-range and
    # infinite ones (the lanes' ranks differ from their indices), all NaN (a zero-count image in
    # the middle), random: the second and third images start at byte offsets 3 modulo 4
    m = disp(3, 37, 50, 8)
    yy, xx = np.meshgrid(np.arange(37), np.arange(50), indexing="ij")
    m[0][(yy + xx) % 2 == 1] = 0.0
    m[0][((yy + xx) % 2 == 1) & (xx % 3 == 0)] = np.inf
    m[0][((yy + xx) % 2 == 1) & (xx % 3 == 1)] = -np.inf
    m[1] = np.nan
    add("mixed_3x37x50", m, 8)
    add("stride2_3x37x50", disp(3, 37, 50, 9), 9, near=0.15, stride=2)
    add("stride3_3x37x50", disp(3, 37, 50, 10), 10, near=0.15, stride=3)
    add("stride64_3x37x50", disp(3, 37, 50, 11), 11, stride=64)       # one record per image
    # depth input: a sparse map of zeros, values exactly at near and far and one ulp outside
    rng = np.random.RandomState(12)
    m = np.zeros((2, 37, 50), F32)
    hit = rng.uniform(size=m.shape) < 0.05
    m[hit] = rng.uniform(1.0, 90.0, int(hit.sum())).astype(F32)
    near, far = F32(1.5), F32(80.0)
    m[0, 0, :4] = near, ulp_down(near), ulp_up(near), -near
    m[0, 36, 46:] = far, ulp_up(far), ulp_down(far), np.inf
    m[1, 17, 20:24] = far, near, ulp_up(far), ulp_down(near)
    add("sparse_depth_2x37x50", m, 12, depth_input=True, near=float(near), far=float(far))
    add("metric_2x37x50", disp(2, 37, 50, 13), 13, depth_scale=5.4, near=1.0, far=80.0)
    add("world_3x37x50", disp(3, 37, 50, 14), 14, T=rigid(3, 14), near=0.15)
    add("world_depth_2x3x5", np.random.RandomState(15).uniform(0.5, 100.0, (2, 3, 5)), 15, T=rigid(2, 15),
        depth_input=True)
    add("2x64x128", disp(2, 64, 128, 16), 16, near=0.15)              # the smallest network feed size
    # more blocks than one pass of the scan takes (1024 threads x 8 counts): the carry
    add("8200x1x1", disp(8200, 1, 1, 17), 17, near=0.15)
    return c


# ---- loaders -----------------------------------------------------------------------------

def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def case(g, name):
    return {k: g[k + "_" + name] for k in ("disp", "inv_K", "K", "depth", "cam", "f64")} | \
        {"floor": float(g["floor_" + name])}
