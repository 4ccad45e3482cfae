"""Makes tests/golden/points/points.npz on the CPU:

    python tests/golden/points/make_points_golden.py --ref REFERENCE_CHECKOUT

Imports the reference's own layers.py (as tests/golden/make_golden.py does) and runs its
unmodified `disp_to_depth(disp, 0.1, 100)` and `BackprojectDepth(B, H, W)(depth, inv_K)` on
the inputs of tests/points_case.golden_cases().  Recorded per case: the inputs, the
reference's depth and camera points (fp32), the same formula evaluated in fp64 from the same
fp32 inputs, and the floor: the maximum over pixels of |reference - fp64| divided by the
point's largest |coordinate|.  Before anything is written the numpy restatement of
tests/points_case.py is measured against all of it, also at 192 x 640 and 375 x 1242 (not
recorded: only their figures are, as `sizes` / `measured`); the figures it prints are the
ones DESIGN §6i quotes.  Only data is written, none of the reference's text.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import points_case as pc  # noqa: E402


def reference_points(ref_layers, disp, inv_K):
    """(depth (B,H,W), cam (B,3,H,W)) fp32 from the reference's layers."""
    B, H, W = disp.shape
    _, depth = ref_layers.disp_to_depth(torch.from_numpy(disp)[:, None], 0.1, 100)
    with torch.no_grad():
        cam = ref_layers.BackprojectDepth(B, H, W)(depth, torch.from_numpy(inv_K))
    assert cam.shape == (B, 4, H * W) and bool((cam[:, 3] == 1).all())
    return depth[:, 0].numpy(), cam[:, :3].reshape(B, 3, H, W).numpy()


def points_f64(disp, inv_K):
    """The written formula in fp64 from the fp32 inputs (the scalars as the fp32 values the
    operator receives)."""
    a, b = (np.float64(v) for v in pc.disp_scalars())
    depth = 1.0 / (b + a * disp.astype(np.float64))
    B, H, W = disp.shape
    k = inv_K.astype(np.float64)
    x = np.arange(W, dtype=np.float64)[None, None, :]
    y = np.arange(H, dtype=np.float64)[None, :, None]
    P = np.empty((B, 3, H, W), np.float64)
    for i in range(3):
        P[:, i] = depth * (k[:, i, 0][:, None, None] * x + k[:, i, 1][:, None, None] * y + k[:, i, 2][:, None, None])
    return P


def relative(a, f64):
    """max over pixels of |a - fp64| / the point's largest |coordinate|."""
    return float((np.abs(a.astype(np.float64) - f64).max(axis=1) / np.abs(f64).max(axis=1)).max())


def measure(ref_layers, name, disp, inv_K, K):
    depth, cam = reference_points(ref_layers, disp, inv_K)
    f64 = points_f64(disp, inv_K)
    floor = relative(cam, f64)
    my_depth = pc.depth_np(disp)
    _, mine = pc.camera_points_np(my_depth, inv_K)
    assert np.array_equal(my_depth.view(np.uint32), depth.view(np.uint32)), name     # depth: bit-equal
    same = float((mine.view(np.uint32) == cam.view(np.uint32)).mean())
    apart = float((np.abs(mine.astype(np.float64) - cam) / np.abs(f64).max(axis=1, keepdims=True)).max())
    my_err = relative(mine, f64)
    rec, _, keep, _ = pc.points_np(disp, pc.colours(*disp.shape, 0), inv_K, far=np.inf)
    assert keep.all()
    u, v = pc.reproject_np(rec, K[0])
    b, y, x = np.nonzero(keep)
    px = float(max(np.abs(u - x).max(), np.abs(v - y).max()))
    print("%-14s depth bit-equal; coordinates bit-equal in %.2f %%, at most %.2e apart (relative); floor "
          "|reference - fp64| %.3e, restatement %.3e (%.2f floors); reprojection within %.2e px" %
          (name, 100 * same, apart, floor, my_err, my_err / floor, px))
    assert my_err <= 4 * floor and px <= 0.01, name
    return depth, cam, f64, floor, np.array([same, apart, floor, my_err, px])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference (its layers.py is imported)")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import layers as ref_layers  # noqa: E402

    out = {"versions": np.array(["numpy " + np.__version__, "torch " + torch.__version__])}
    names = []
    for name, (disp, inv_K, K) in pc.golden_cases().items():
        names.append(name)
        depth, cam, f64, floor, _ = measure(ref_layers, name, disp, inv_K, K)
        out.update({"disp_" + name: disp, "inv_K_" + name: inv_K, "K_" + name: K, "depth_" + name: depth,
                    "cam_" + name: cam, "f64_" + name: f64, "floor_" + name: np.float64(floor)})
    out["names"] = np.array(names)

    # the network's feed size and KITTI's image size: measured, their figures recorded
    sizes, figures = [], []
    for H, W, seed in ((192, 640, 10), (375, 1242, 11)):
        disp = np.random.RandomState(seed).uniform(0.0, 1.0, (1, H, W)).astype(np.float32)
        K, inv_K = pc.intrinsics(H, W)
        figures.append(measure(ref_layers, "%dx%d" % (H, W), disp, inv_K, K)[4])
        sizes.append((H, W))
    out["sizes"] = np.array(sizes, np.int32)
    out["measured"] = np.stack(figures)     # per size: bit-equal share, apart, floor, restatement, px

    path = os.path.join(HERE, "points.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
