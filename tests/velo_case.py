"""The yardstick of the velodyne projection tests: a vectorised numpy restatement of the
reference's kitti_utils.generate_depth_map (kitti_utils.py:46-98), formulated with a
stable sort and ufunc.at — not with the kernel's per-pixel atomic records — plus writers
of synthetic calibration files and scans.  tests/golden/velo/make_velo_golden.py checks
the restatement bit-equal to the reference's own function before it records the golden.
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "velo", "velo_depth.npz")
SIZES = ((13, 41), (37, 124))   # the golden's image sizes, scene i at SIZES[i]
CAMS = (2, 3)


def project(points, P, blas=False):
    """The kept points' (q0 / q2, q1 / q2, q2, x) in fp64 and their indices.  `blas`: the
    reference's np.dot (whatever summation order the host's BLAS has) instead of the
    written order ((P0*x + P1*y) + P2*z) + P3 of separately rounded products."""
    pts = np.asarray(points, dtype=np.float32)
    keep = np.flatnonzero(pts[:, 0] >= 0)
    xyz = pts[keep, :3].astype(np.float64)
    P = np.asarray(P, dtype=np.float64)
    with np.errstate(all="ignore"):
        if blas:
            hom = np.concatenate([xyz, np.ones((len(keep), 1))], 1)
            q = np.dot(P, hom.T).T
        else:
            q = np.stack([((P[r, 0] * xyz[:, 0] + P[r, 1] * xyz[:, 1]) + P[r, 2] * xyz[:, 2]) + P[r, 3]
                          for r in range(3)], 1)
        return q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], q[:, 2], xyz[:, 0], keep


def valid_points(points, P, H, W, vel_depth=False, blas=False):
    """(u, v, depth) of the valid points in point order: int64, int64, fp64."""
    fu, fv, q2, x, _ = project(points, P, blas)
    with np.errstate(all="ignore"):
        u, v = np.round(fu) - 1, np.round(fv) - 1
        ok = (u >= 0) & (v >= 0) & (u < W) & (v < H)   # in fp64, before any integer conversion
    d = x if vel_depth else q2
    return u[ok].astype(np.int64), v[ok].astype(np.int64), d[ok]


def depth_map_np(points, P, H, W, vel_depth=False, blas=False):
    """Rules 1-7 of the reference for one frame -> fp64 (H, W)."""
    u, v, d = valid_points(points, P, H, W, vel_depth, blas)
    depth = np.zeros(H * W, dtype=np.float64)
    n = len(d)
    if n:
        pix = v * W + u
        # the fancy assignment: the last point of every pixel
        last = np.full(H * W, -1, dtype=np.int64)
        np.maximum.at(last, pix, np.arange(n))
        hit = last >= 0
        depth[hit] = d[last[hit]]
        # duplicates under the reference's sub2ind key: the pixel of a group's first point
        # gets the group's minimum
        key = v * (W - 1) + u - 1
        order = np.argsort(key, kind="stable")
        ks = key[order]
        start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        count = np.diff(np.r_[start, n])
        gmin = np.minimum.reduceat(d[order], start)
        first = order[start]                      # stable: the smallest index of the group
        dup = count > 1
        depth[pix[first[dup]]] = gmin[dup]
    depth[depth < 0] = 0
    return depth.reshape(H, W)


def pixel_min_np(points, P, H, W, vel_depth=False):
    """What the reference does NOT compute: the plain per-pixel minimum (to show that a
    case exercises the sub2ind quirk)."""
    u, v, d = valid_points(points, P, H, W, vel_depth)
    depth = np.full(H * W, np.inf)
    np.minimum.at(depth, v * W + u, d)
    depth[np.isinf(depth)] = 0
    depth[depth < 0] = 0
    return depth.reshape(H, W)


def half_integer_margin(points, P, H, W):
    """The smallest distance of a valid point's unrounded u or v to a half-integer."""
    fu, fv, _, _, _ = project(points, P)
    with np.errstate(all="ignore"):
        u, v = np.round(fu) - 1, np.round(fv) - 1
        ok = (u >= 0) & (v >= 0) & (u < W) & (v < H)
    both = np.concatenate([fu[ok], fv[ok]])
    if both.size == 0:
        return np.inf
    return float(np.abs(np.abs(both - np.floor(both)) - 0.5).min())


# ---- synthetic calibration and scans ----------------------------------------------------

def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _line(key, values):
    return key + ": " + " ".join("%.12e" % float(v) for v in np.ravel(values))


def calib_texts(H, W, seed=0):
    """(calib_cam_to_cam.txt, calib_velo_to_cam.txt) of a KITTI-like rig with a W x H
    rectified image: velodyne x forward / y left / z up -> camera x right / y down / z
    forward with small perturbing rotations, cameras 2 and 3 a baseline apart."""
    rng = np.random.default_rng(seed)
    f = 0.58 * W
    cx, cy = 0.5 * W + rng.uniform(-1, 1), 0.5 * H + rng.uniform(-1, 1)
    cam = ["calib_time: 09-Jan-2012 13:57:47", _line("corner_dist", [9.95e-2])]
    rect = _rot(*rng.uniform(-0.01, 0.01, 3))
    for c in range(4):
        base = (0.0, 0.0, -0.06 * f, 0.47 * f)[c]   # P[0, 3] = -f * baseline
        P = np.array([[f, 0, cx, base], [0, f, cy, rng.uniform(-0.3, 0.3) if c else 0.0],
                      [0, 0, 1, rng.uniform(-0.004, 0.004) if c else 0.0]])
        cam.append(_line("S_rect_%02d" % c, [W, H]))
        cam.append(_line("R_rect_%02d" % c, rect if c == 0 else _rot(*rng.uniform(-0.01, 0.01, 3))))
        cam.append(_line("P_rect_%02d" % c, P))
    axes = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])
    R = _rot(*rng.uniform(-0.02, 0.02, 3)) @ axes
    T = np.array([rng.uniform(-0.02, 0.02), -0.07, -0.27])
    velo = ["calib_time: 15-Mar-2012 11:37:16", _line("R", R), _line("T", T),
            _line("delta_f", [0, 0]), _line("delta_c", [0, 0])]
    return "\n".join(cam) + "\n", "\n".join(velo) + "\n"


def write_calib_dir(path, texts):
    os.makedirs(path, exist_ok=True)
    for name, text in zip(("calib_cam_to_cam.txt", "calib_velo_to_cam.txt"), texts):
        with open(os.path.join(path, name), "w") as fh:
            fh.write(text)
    return path


def make_scan(n, seed=0, spread=1.15):
    """A LiDAR-like fp32 (n, 4) scan: most points in front within (a little more than) the
    field of view of `calib_texts`, some behind the sensor (x < 0), some far off frame and
    some so close that the camera's z is negative (the rig's T puts the camera 0.27 in
    front of the sensor)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.5, 60.0, n)
    y = x * rng.uniform(-0.9, 0.9, n) * spread
    z = x * rng.uniform(-0.3, 0.3, n) * spread - 0.05
    kind = rng.uniform(0, 1, n)
    behind, off, near = kind < 0.08, (kind >= 0.08) & (kind < 0.14), (kind >= 0.14) & (kind < 0.22)
    x[behind] = -x[behind]
    y[off] = y[off] * 4 + 50.0
    x[near] = rng.uniform(0.0, 0.26, near.sum())
    y[near] = rng.uniform(-0.2, 0.2, near.sum())
    z[near] = rng.uniform(-0.1, 0.1, near.sum())
    pts = np.stack([x, y, z, rng.uniform(0, 1, n)], 1).astype(np.float32)
    return pts


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)
