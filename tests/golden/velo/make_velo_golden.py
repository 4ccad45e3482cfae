"""Capture tests/golden/velo/velo_depth.npz from the reference's own
kitti_utils.generate_depth_map (kitti_utils.py:46-98), unmodified, on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/velo/make_velo_golden.py [--ref /root/reference]

The reference uses `np.int`, which numpy 2 no longer has: it is set to `int` here before
the import.  Two synthetic rigs (13 x 41 and 37 x 124 images) are written as KITTI
calibration text, one scan each (4 000 and 20 000 points, with points behind the sensor,
off frame and with negative camera depth); recorded are the scans, the calibration texts,
what the reference's read_calib_file makes of them, its projection matrices and its maps
for cameras 2 and 3 with vel_depth both ways.  Before saving, three things are confirmed:

  * tests/velo_case.py's restatement is bit-equal to the reference (fp64, with the
    reference's np.dot; and as fp32 with the written summation order the kernel uses);
  * every map differs from a plain per-pixel minimum in column 0 or W-1 (the sub2ind
    quirk is exercised);
  * no valid point's unrounded u or v lies within 1e-9 of a half-integer, so a last-bit
    difference in the projection cannot move a point to another pixel: nothing has to be
    left out of the comparison (the seeds were chosen for that).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # tests: velo_case

import velo_case as vc  # noqa: E402

POINTS = (4000, 20000)
SEEDS = (3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=vc.GOLDEN)
    args = ap.parse_args()
    np.int = int   # numpy < 1.24 name the reference still uses
    sys.path.insert(0, args.ref)
    import kitti_utils as ref

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, ((H, W), n, seed) in enumerate(zip(vc.SIZES, POINTS, SEEDS)):
            texts = vc.calib_texts(H, W, seed)
            cdir = vc.write_calib_dir(os.path.join(tmp, "rig%d" % i), texts)
            pts = vc.make_scan(n, seed)
            pts[:, 3] = 0     # the reflectance is ignored; zeros compress
            scan = os.path.join(tmp, "scan%d.bin" % i)
            pts.tofile(scan)
            out["points_%d" % i] = pts
            out["cam2cam_%d" % i], out["velo2cam_%d" % i] = np.array(texts[0]), np.array(texts[1])
            cam2cam = ref.read_calib_file(os.path.join(cdir, "calib_cam_to_cam.txt"))
            velo = ref.read_calib_file(os.path.join(cdir, "calib_velo_to_cam.txt"))
            assert cam2cam["S_rect_02"].tolist() == [W, H]
            for k in ("S_rect_02", "R_rect_00", "P_rect_02", "P_rect_03"):
                out["calib_%d_%s" % (i, k)] = cam2cam[k]
            for k in ("R", "T"):
                out["calib_%d_%s" % (i, k)] = velo[k]
            v2c = np.eye(4)
            v2c[:3, :3], v2c[:3, 3] = velo["R"].reshape(3, 3), velo["T"]
            rect = np.eye(4)
            rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
            for cam in vc.CAMS:
                P = np.dot(np.dot(cam2cam["P_rect_0%d" % cam].reshape(3, 4), rect), v2c)
                out["P_%d_cam%d" % (i, cam)] = P
                margin = vc.half_integer_margin(pts, P, H, W)
                assert margin > 1e-9, (i, cam, margin)
                for vel in (False, True):
                    want = ref.generate_depth_map(cdir, scan, cam, vel)
                    assert want.shape == (H, W) and want.dtype == np.float64
                    same = vc.depth_map_np(pts, P, H, W, vel, blas=True)
                    assert np.array_equal(same.view(np.uint64), want.view(np.uint64)), (i, cam, vel)
                    mine = vc.depth_map_np(pts, P, H, W, vel).astype(np.float32)
                    want32 = want.astype(np.float32)
                    assert np.array_equal(mine.view(np.uint32), want32.view(np.uint32)), (i, cam, vel)
                    plain = vc.pixel_min_np(pts, P, H, W, vel).astype(np.float32)
                    quirk = np.argwhere(plain != want32)
                    assert len(quirk) and set(quirk[:, 1]) <= {0, W - 1}, (i, cam, vel, quirk)
                    out["depth_%d_cam%d_vel%d" % (i, cam, int(vel))] = want32
                    print("scene %d cam %d vel_depth %d: %d occupied, %d valid points of negative depth, %d quirk "
                          "pixels, half-integer margin %.3e" % (i, cam, vel, np.count_nonzero(want32),
                                                                int((vc.valid_points(pts, P, H, W, vel)[2] < 0).sum()),
                                                                len(quirk), margin))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
