"""The yardstick of the pose-evaluation tests: a numpy fp64 restatement of md2_pose_ate
(include/md2hot.h; the reference's evaluate_pose.py:104-125) in the kernel's written
order — every product and sum one separately rounded fp64 operation on numpy scalars or
arrays, explicit four-term sums, the cofactor inverse, the fixed-shape reduction; no
np.dot, np.linalg or np.mean — a second variant with the rigid transpose inverse (what the
kernel must NOT compute; only the golden maker and one CPU test use it), and the
synthetic drive and predictions.  tests/golden/pose_eval/make_pose_eval_golden.py
measures the restatement against the reference's own functions before it records the
golden.
"""
from __future__ import annotations

import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_eval", "pose_eval.npz")
FRAMES = (6, 300)      # the golden's sequences, sequence i has FRAMES[i] frames
SEEDS = (11, 12)
LANES = 256


# ---- the restatement ---------------------------------------------------------------------

def affine_inverse(m):
    """General inverse of [A | t; 0 0 0 1]; m (..., 3, 4) -> (..., 3, 4)."""
    a, b, c = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    d, e, f = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    g, h, k = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    c00, c01, c02 = e * k - f * h, f * g - d * k, d * h - e * g
    c10, c11, c12 = c * h - b * k, a * k - c * g, b * g - a * h
    c20, c21, c22 = b * f - c * e, c * d - a * f, a * e - b * d
    det = (a * c00 + b * c01) + c * c02
    out = np.empty_like(m)
    for r, row in enumerate(((c00, c10, c20), (c01, c11, c21), (c02, c12, c22))):
        for j in range(3):
            out[..., r, j] = row[j] / det
    x, y, z = m[..., 0, 3], m[..., 1, 3], m[..., 2, 3]
    for r in range(3):
        out[..., r, 3] = -((out[..., r, 0] * x + out[..., r, 1] * y) + out[..., r, 2] * z)
    return out


def rigid_inverse(m):
    """The shortcut [R^T | -R^T t]: exact only for an orthonormal R."""
    out = np.empty_like(m)
    for r in range(3):
        for j in range(3):
            out[..., r, j] = m[..., j, r]
    x, y, z = m[..., 0, 3], m[..., 1, 3], m[..., 2, 3]
    for r in range(3):
        out[..., r, 3] = -((out[..., r, 0] * x + out[..., r, 1] * y) + out[..., r, 2] * z)
    return out


def mul34(A, B):
    """Top three rows of A . B: A (..., 3, 4), B (..., 4, 4), four-term sums."""
    out = np.empty(np.broadcast_shapes(A.shape[:-2], B.shape[:-2]) + (3, 4), dtype=np.float64)
    for r in range(3):
        for c in range(4):
            out[..., r, c] = ((A[..., r, 0] * B[..., 0, c] + A[..., r, 1] * B[..., 1, c])
                              + A[..., r, 2] * B[..., 2, c]) + A[..., r, 3] * B[..., 3, c]
    return out


def with_bottom_row(m):
    out = np.zeros(m.shape[:-2] + (4, 4), dtype=np.float64)
    out[..., :3, :] = m
    out[..., 3, 3] = 1.0
    return out


def local_poses(gt, inverse=affine_inverse):
    """gt (M, 3, 4) -> L (M-1, 4, 4): L_i = inv(inv(G_{i-1}) . G_i)."""
    gt = np.asarray(gt, dtype=np.float64)
    return with_bottom_row(inverse(mul34(inverse(gt[:-1]), with_bottom_row(gt[1:]))))


def dump_xyz(transforms):
    """(n, 4, 4) fp64 -> (n + 1, 3) points."""
    C = np.zeros((3, 4), dtype=np.float64)
    C[0, 0] = C[1, 1] = C[2, 2] = 1.0
    pts = [np.zeros(3, dtype=np.float64)]
    for T in transforms:
        C = mul34(C, T)
        pts.append(C[:, 3].copy())
    return np.array(pts)


def compute_ate(g, p):
    with np.errstate(all="ignore"):
        p = p + (g[0] - p[0])[None, :]
        num, den = np.float64(0.0), np.float64(0.0)
        for k in range(len(g)):
            for c in range(3):
                num = num + g[k, c] * p[k, c]
                den = den + p[k, c] * p[k, c]
        scale = num / den
        sse = np.float64(0.0)
        for k in range(len(g)):
            for c in range(3):
                e = p[k, c] * scale - g[k, c]
                sse = sse + e * e
        return np.sqrt(sse) / np.float64(len(g))


def fixed_sum(x):
    """256 lanes, lane j adds x[j], x[j + 256], ... in rising order from 0.0; then strides
    128, 64, ..., 1 fold lane j + stride into lane j."""
    lanes = np.zeros(LANES, dtype=np.float64)
    for start in range(0, len(x), LANES):
        chunk = x[start:start + LANES]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    half = LANES // 2
    while half:
        lanes[:half] = lanes[:half] + lanes[half:2 * half]
        half //= 2
    return lanes[0]


def stats_np(ates):
    with np.errstate(all="ignore"):
        n = np.float64(len(ates))
        mean = fixed_sum(ates) / n
        dev = ates - mean
        return np.array([mean, np.sqrt(fixed_sum(dev * dev) / n)])


def trajectory_ate_np(pred, gt, track_length=5, inverse=affine_inverse):
    """One sequence: pred (M-1, 4, 4) fp32, gt (M, 3, 4) fp64 -> (ates (M-1,), stats (2,))."""
    pred = np.asarray(pred, dtype=np.float32).astype(np.float64)
    L = local_poses(gt, inverse)
    assert len(pred) == len(L)
    ates = np.array([compute_ate(dump_xyz(L[i:i + track_length - 1]), dump_xyz(pred[i:i + track_length - 1]))
                     for i in range(len(L))])
    return ates, stats_np(ates)


# ---- synthetic drive and predictions -----------------------------------------------------

def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def drive_text(frames, seed=0, origin=(312.5, -7.25, 468.0), yaw=0.7):
    """A smooth forward drive in KITTI's pose format (camera x right, y down, z forward;
    one 3x4 camera-to-world per line, %.6e): about a metre per frame along a slowly turning
    heading, a few hundred metres from the origin, as the later frames of a KITTI sequence
    are.  Six decimals leave the rotations orthonormal to about 1e-7 only."""
    rng = np.random.default_rng(seed)
    pos, heading = np.array(origin, dtype=np.float64), yaw
    pitch = roll = 0.0
    lines = []
    for i in range(frames):
        R = _rot(pitch, heading, roll)
        lines.append(" ".join("%.6e" % v for v in np.concatenate([R, pos[:, None]], 1).ravel()))
        speed = 1.0 + 0.3 * np.sin(0.05 * i) + rng.normal(0, 0.02)
        pos = pos + R @ np.array([rng.normal(0, 0.005), rng.normal(0, 0.005), speed])
        heading += 0.01 * np.sin(0.02 * i + 1.0) + rng.normal(0, 0.001)
        pitch = 0.01 * np.sin(0.11 * i) + rng.normal(0, 0.0005)
        roll = 0.008 * np.cos(0.07 * i) + rng.normal(0, 0.0005)
    return "\n".join(lines) + "\n"


def parse_text(text):
    return np.loadtxt(io.StringIO(text)).reshape(-1, 3, 4)


def predictions(gt, seed=0, scale=0.031, noise=0.04):
    """fp32 (axisangle (M-1, 1, 3), translation (M-1, 1, 3)) of a pose network for the drive
    `gt`: the local motion of every frame pair as axis-angle and translation, the
    translation at the arbitrary scale of monocular training, both with noise."""
    rng = np.random.default_rng(seed + 1000)
    L = local_poses(gt)
    R = L[:, :3, :3]
    w = 0.5 * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)  # sin(a) axis
    s = np.linalg.norm(w, axis=1, keepdims=True)
    aa = w * np.where(s > 1e-12, np.arcsin(np.minimum(s, 1.0)) / np.maximum(s, 1e-300), 1.0)
    aa = aa + rng.normal(0, 5e-4, aa.shape)
    t = L[:, :3, 3] * scale
    t = t * (1 + rng.normal(0, noise, (len(t), 1))) + rng.normal(0, noise * scale * 0.3, t.shape)
    return aa[:, None, :].astype(np.float32), t[:, None, :].astype(np.float32)


def identity_poses(n):
    out = np.zeros((n, 4, 4), dtype=np.float32)
    out[:, range(4), range(4)] = 1
    return out


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)
