"""Capture tests/golden/pose_eval/pose_eval.npz from the reference's own evaluate_pose.py
(dump_xyz, compute_ate) and layers.transformation_from_parameters, unmodified, on the CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/pose_eval/make_pose_eval_golden.py [--ref /root/reference]

The reference is imported with the module stubs of tests/golden/make_golden.py (its
`datasets` pulls in skimage, which is not installed).  For two synthetic drives
(tests/pose_eval_case.py: 6 and 300 frames, written in KITTI's %.6e pose format and read
back, fp32 axis-angle / translation predictions) lines 104-125 of evaluate_pose.py are
repeated around the reference's functions with np.loadtxt, np.linalg.inv and np.dot,
unmodified in meaning.  Recorded per sequence: the pose text, what np.loadtxt makes of it,
axisangle, translation, the fp32 pred_poses, the reference's ates, mean, std and printed
line.  Before saving, measured, confirmed and recorded:

  * floor: the largest relative difference between tests/pose_eval_case.py's cofactor
    restatement and the reference over all ATEs, means and stds;
  * rigid: the same for the rigid-inverse variant, which must miss the reference by at
    least 100 x floor (the fixture exercises the trap);
  * no golden ATE is nan or below 1e-4, so relative bars are meaningful;
  * ulp_bar: 4 x the largest relative change of any ATE, mean or std when every element of
    pred_poses moves by one fp32 ulp in a random direction (8 draws per sequence): the bar
    of the end-to-end test, whose transforms come from another implementation of
    transformation_from_parameters.
"""
from __future__ import annotations

import argparse
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/golden: make_golden
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # tests: pose_eval_case

import pose_eval_case as pc  # noqa: E402


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=pc.GOLDEN)
    args = ap.parse_args()
    from make_golden import _stub_modules
    _stub_modules()
    sys.path.insert(0, args.ref)
    import evaluate_pose as ref
    import layers as ref_layers

    out = {}
    floor = rigid = ulp = 0.0
    for s, (frames, seed) in enumerate(zip(pc.FRAMES, pc.SEEDS)):
        text = pc.drive_text(frames, seed)
        gt34 = np.loadtxt(io.StringIO(text)).reshape(-1, 3, 4)
        aa, tr = pc.predictions(gt34, seed)
        pred_poses = ref_layers.transformation_from_parameters(torch.from_numpy(aa), torch.from_numpy(tr)).cpu().numpy()
        assert pred_poses.dtype == np.float32 and pred_poses.shape == (frames - 1, 4, 4)

        # evaluate_pose.py:105-125
        gt_global_poses = gt34
        gt_global_poses = np.concatenate(
            (gt_global_poses, np.zeros((gt_global_poses.shape[0], 1, 4))), 1)
        gt_global_poses[:, 3, 3] = 1
        gt_xyzs = gt_global_poses[:, :3, 3]
        gt_local_poses = []
        for i in range(1, len(gt_global_poses)):
            gt_local_poses.append(
                np.linalg.inv(np.dot(np.linalg.inv(gt_global_poses[i - 1]), gt_global_poses[i])))
        ates = []
        num_frames = gt_xyzs.shape[0]
        track_length = 5
        for i in range(0, num_frames - 1):
            local_xyzs = np.array(ref.dump_xyz(pred_poses[i:i + track_length - 1]))
            gt_local_xyzs = np.array(ref.dump_xyz(gt_local_poses[i:i + track_length - 1]))
            ates.append(ref.compute_ate(gt_local_xyzs, local_xyzs))
        line = "\n   Trajectory error: {:0.3f}, std: {:0.3f}\n".format(np.mean(ates), np.std(ates))

        ates = np.array(ates)
        want = np.concatenate([ates, [np.mean(ates), np.std(ates)]])
        assert np.isfinite(want).all() and ates.min() >= 1e-4, ates.min()
        mine = np.concatenate(pc.trajectory_ate_np(pred_poses, gt34))
        bad = np.concatenate(pc.trajectory_ate_np(pred_poses, gt34, inverse=pc.rigid_inverse))
        floor, rigid = max(floor, rel(mine, want)), max(rigid, rel(bad, want))
        rng = np.random.default_rng(seed + 2000)
        for _ in range(8):
            up = rng.integers(0, 2, pred_poses.shape).astype(bool)
            moved = np.where(up, np.nextafter(pred_poses, np.float32(np.inf)), np.nextafter(pred_poses, np.float32(-np.inf)))
            ulp = max(ulp, rel(np.concatenate(pc.trajectory_ate_np(moved.astype(np.float32), gt34)), mine))
        print("sequence %d: %d frames, ates %.4f .. %.4f, mean %.6f std %.6f, line %r" %
              (s, frames, ates.min(), ates.max(), want[-2], want[-1], line))
        out.update({"pose_text_%d" % s: np.array(text), "gt_%d" % s: gt34, "axisangle_%d" % s: aa,
                    "translation_%d" % s: tr, "pred_poses_%d" % s: pred_poses, "ates_%d" % s: ates,
                    "mean_%d" % s: want[-2], "std_%d" % s: want[-1], "line_%d" % s: np.array(line)})
    print("floor %.3e  rigid %.3e (%.0f x floor)  ulp_bar %.3e" % (floor, rigid, rigid / floor, 4 * ulp))
    assert floor > 0 and rigid >= 100 * floor, (floor, rigid)
    out.update(floor=np.float64(floor), rigid=np.float64(rigid), ulp_bar=np.float64(4 * ulp))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
