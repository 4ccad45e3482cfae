"""Capture tests/golden/depth_eval/depth_eval_monitor.npz from the reference's own
Trainer.compute_depth_losses (trainer.py:498-526), unmodified and called unbound, on the
CPU in fp32, at its fixed 375 x 1242 ground-truth size.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/depth_eval/make_depth_eval_golden.py [--ref /root/reference]

Inputs: B = 2 sigmoid disparity maps of 24 x 80 (outputs[("depth", 0, 0)] is the
reference's disp_to_depth of them) and LiDAR-like ground truth at ~3 % density, stored
sparsely (flat indices + values).  Pixels whose fp64 threshold ratio lies within 1e-4 of
1.25^k are removed first (tests/eval_case.py clear_thresholds), so a1..a3 do not depend on
the evaluation's precision.

The fixture has a folder of its own because tests/golden_io.py reads every .npz directly
under tests/golden/ as a hot-path case.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/golden: make_golden
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # tests: eval_case

from eval_case import clear_thresholds, make_inputs  # noqa: E402
from make_golden import import_reference             # noqa: E402

NAMES = ["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "depth_eval_monitor.npz"))
    args = ap.parse_args()
    ref_trainer, ref_layers = import_reference(args.ref)
    sig, _, gt = make_inputs(B=2, h=24, w=80, GH=375, GW=1242, seed=11, density=0.03)
    gt, removed, before = clear_thresholds(sig, gt, mode="monitor")
    assert removed < 0.01 * before, (removed, before)
    _, depth = ref_layers.disp_to_depth(torch.from_numpy(sig), 0.1, 100.0)
    me = types.SimpleNamespace(depth_metric_names=NAMES)
    losses = {}
    ref_trainer.Trainer.compute_depth_losses(me, {"depth_gt": torch.from_numpy(gt).unsqueeze(1)},
                                             {("depth", 0, 0): depth}, losses)
    metrics = np.array([float(losses[n]) for n in NAMES], dtype=np.float32)
    idx = np.flatnonzero(gt).astype(np.int32)
    np.savez_compressed(args.out, sig=sig, gt_shape=np.array(gt.shape, dtype=np.int32), gt_index=idx,
                        gt_value=gt.reshape(-1)[idx], metrics=metrics, removed=np.array([removed, before]))
    print(args.out, os.path.getsize(args.out), "bytes;", idx.size, "gt values; removed", removed, "of", before)
    print(dict(zip(NAMES, metrics.tolist())))


if __name__ == "__main__":
    main()
