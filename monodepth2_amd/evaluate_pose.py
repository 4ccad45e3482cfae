"""KITTI odometry pose evaluation (the reference's evaluate_pose.py) on the device.

    python -m monodepth2_amd.evaluate_pose --eval_split odom_9 --ext_poses_to_eval poses.npy \\
        --gt_poses 09.txt

`evaluate(opt)` reports the reference's one number for a pose network trained on the
odometry split: the 5-frame absolute trajectory error on sequence 09 or 10, mean and
standard deviation.  The reference's formulation (evaluate_pose.py:104-125: two LAPACK
inverses per frame, then a Python loop of np.dot chains per snippet, on the host) runs as
the fused fp64 HIP operator of `pose_eval_ops.trajectory_ate`, one call, one device-to-host
copy at the end.

Ground truth: --gt_poses, a KITTI `poses/NN.txt` (default <data_path>/poses/NN.txt).
Predictions: --ext_poses_to_eval, the (N,4,4) float32 `poses.npy` this command and the
reference write; or the checkpoint in --load_weights_folder (pose_encoder.pth, pose.pth)
run by `predict_poses` on images the caller loaded; or, as in the reference, that
checkpoint run on the frames test_files_09.txt / test_files_10.txt name under --data_path
(--split_dir, default splits/odom/ beside this package; the lists are not shipped):
datasets.KITTIOdomDataset decodes frames k and k + 1 of every line, loader.BatchLoader
(list order, --batch_size lines per pass, the partial last batch included) resizes them to
--height x --width on the device, bit-equal to the reference's PIL pipeline.

    python -m monodepth2_amd.evaluate_pose --eval_split odom_9 --load_weights_folder W \\
        --data_path KITTI_ODOM --split_dir splits/odom

Out of scope: shipping the split lists (a missing one is an `options.SplitListMissing`, a
FileNotFoundError that names --split_dir and, as the refusal of this route was before it
existed, a NotImplementedError), and the `posecnn` and `shared` pose models, which the
reference's evaluate_pose supports neither.
"""
from __future__ import annotations

import os
from typing import Dict

import numpy as np
import torch

from . import networks
from .datasets import readlines
from .options import MonodepthOptions, SplitListMissing
from .pose_eval_ops import trajectory_ate
from .pose_ops import poses_to_transforms

TRACK_LENGTH = 5   # evaluate_pose.py:118
SPLITS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "splits")


def load_gt_poses(path: str) -> np.ndarray:
    """A KITTI poses file, 12 numbers per line (the 3x4 camera-to-world of each frame),
    as (M, 3, 4) float64 (evaluate_pose.py:105)."""
    rows = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if rows.shape[1] != 12:
        raise ValueError("{}: expected 12 numbers per line, found {}".format(path, rows.shape[1]))
    return rows.reshape(-1, 3, 4)


def _pose_batch(pose_encoder, pose_decoder, first: torch.Tensor, second: torch.Tensor) -> torch.Tensor:
    """One pass of evaluate_pose.py:94-100 on n frame pairs (n,3,H,W) each: (n,4,4).  The
    caller holds eval mode and no_grad."""
    pair = [first.contiguous(), second.contiguous()]
    axisangle, translation = pose_decoder([pose_encoder([pair])])
    aa, tr = axisangle[:, 0, 0].float().unsqueeze(0), translation[:, 0, 0].float().unsqueeze(0)
    return poses_to_transforms(aa, tr, [False])[0]


def _predict_pairs(pose_encoder, pose_decoder, pairs) -> torch.Tensor:
    """`_pose_batch` over an iterable of (first, second) frame batches, in eval mode under
    no_grad; the modules' training flags are restored."""
    was = pose_encoder.training, pose_decoder.training
    pose_encoder.eval()
    pose_decoder.eval()
    out = []
    try:
        with torch.no_grad():
            for first, second in pairs:
                out.append(_pose_batch(pose_encoder, pose_decoder, first, second))
    finally:
        pose_encoder.train(was[0])
        pose_decoder.train(was[1])
    return torch.cat(out)


def predict_poses(pose_encoder, pose_decoder, images: torch.Tensor, batch_size: int = 16) -> torch.Tensor:
    """The transforms between consecutive frames of `images` (M,3,H,W), in [0,1], one
    sequence: evaluate_pose.py:89-100.  Frames i and i+1 go through the pose encoder
    concatenated on the channel axis, eval mode, no_grad, `batch_size` pairs per pass; the
    first predicted frame's axis-angle and translation become 4x4 transforms, not inverted,
    in one launch per batch (pose_ops.poses_to_transforms).  Returns (M-1,4,4) float32 on
    the device of `images`.  Fused ops that decline eval mode fall back to their modules
    on their own; nothing is forced.  The modules' training flags are restored."""
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 2:
        raise ValueError(f"images must be (M, 3, H, W) with M >= 2, got {tuple(images.shape)}")
    last = images.shape[0] - 1

    def pairs():
        for i in range(0, last, batch_size):
            n = min(batch_size, last - i)
            yield images[i:i + n], images[i + 1:i + 1 + n]

    return _predict_pairs(pose_encoder, pose_decoder, pairs())


def split_lines(opt, sequence_id: int):
    """The lines of test_files_NN.txt in --split_dir (default splits/odom/ beside this
    package, where the reference keeps them; the lists are not shipped)."""
    folder = getattr(opt, "split_dir", None) or os.path.join(SPLITS_DIR, "odom")
    path = os.path.join(folder, "test_files_{:02d}.txt".format(sequence_id))
    if not os.path.isfile(path):
        raise SplitListMissing(
            "no split list at {}: evaluating the frames under --data_path needs it, and the split lists are not "
            "shipped with this package (shipping them is out of scope); pass --split_dir DIR with "
            "DIR/test_files_09.txt and DIR/test_files_10.txt (the reference's splits/odom/ folder)".format(path))
    return readlines(path)


def predict_from_disk(pose_encoder, pose_decoder, opt, lines, device) -> torch.Tensor:
    """evaluate_pose.py:60-102 from --data_path: every line's frames k and k + 1, decoded by
    datasets.KITTIOdomDataset and resized to --height x --width on the device
    (loader.BatchLoader in list order, --batch_size lines per pass, the partial last batch
    included; scale 0 only), then the per-batch body of `predict_poses`.  The reference
    feeds `color_aug`, which is `color` when is_train is False."""
    from .datasets import KITTIOdomDataset
    from .loader import BatchLoader
    from .pack import open_pack
    dataset = KITTIOdomDataset(opt.data_path, lines, opt.height, opt.width, [0, 1], 1, is_train=False,
                               img_ext=".png" if opt.png else ".jpg")
    loader = BatchLoader(dataset, opt.batch_size, shuffle=False, drop_last=False, num_workers=opt.num_workers,
                         device=device, device_decode=getattr(opt, "device_decode", False), pack=open_pack(opt),
                         device_png=getattr(opt, "device_png", False))
    try:
        return _predict_pairs(pose_encoder, pose_decoder,
                              ((batch[("color_aug", 0, 0)], batch[("color_aug", 1, 0)]) for batch in loader))
    finally:
        loader.close()


def evaluate_poses(pred_poses, gt_global_poses, track_length: int = TRACK_LENGTH, device=None) -> Dict[str, object]:
    """evaluate_pose.py:106-125 for one sequence: `pred_poses` (M-1,4,4) float32 and
    `gt_global_poses` (M,3,4) float64, numpy or torch.  Returns {"ates": (M-1,) float64,
    "mean", "std"}; one device-to-host copy at the end."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def to_dev(a, dtype, what):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype != dtype:
            raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
        return t.to(device)

    pred = to_dev(pred_poses, torch.float32, "pred_poses")
    gt = to_dev(gt_global_poses, torch.float64, "gt_global_poses")
    if gt.dim() != 3 or gt.shape[0] < 2 or pred.dim() != 3 or pred.shape[0] != gt.shape[0] - 1:
        raise ValueError(f"{tuple(gt.shape)} ground-truth poses need ({max(gt.shape[0] - 1, 0)}, 4, 4) predictions, "
                         f"got {tuple(pred.shape)}")
    ates, stats = trajectory_ate(pred, gt, None, track_length)
    res = torch.cat([ates, stats.reshape(-1)]).cpu().numpy()   # the one synchronisation
    return {"ates": res[:-2], "mean": float(res[-2]), "std": float(res[-1])}


def format_results(res) -> str:
    """The reference's line (evaluate_pose.py:125)."""
    return "\n   Trajectory error: {:0.3f}, std: {:0.3f}\n".format(res["mean"], res["std"])


def load_networks(folder: str, num_layers: int, device):
    """pose_encoder.pth / pose.pth of a checkpoint folder (evaluate_pose.py:69-76)."""
    pose_encoder = networks.ResnetEncoder(num_layers, False, 2)
    pose_encoder.load_state_dict(torch.load(os.path.join(folder, "pose_encoder.pth"), map_location=device,
                                            weights_only=True))
    pose_decoder = networks.PoseDecoder(pose_encoder.num_ch_enc, 1, 2)
    pose_decoder.load_state_dict(torch.load(os.path.join(folder, "pose.pth"), map_location=device,
                                            weights_only=True))
    return pose_encoder.to(device), pose_decoder.to(device)


def evaluate(opt, images: torch.Tensor = None):
    """evaluate_pose.py:49-129.  Predictions come from --ext_poses_to_eval (poses.npy), or
    from the checkpoint in --load_weights_folder run on `images` (M,3,H,W), the frames of
    the sequence in order, or, without them, on the frames test_files_NN.txt names under
    --data_path (`predict_from_disk`); then poses.npy is saved there, as the reference does."""
    if opt.eval_split not in ("odom_9", "odom_10"):
        raise SystemExit("eval_split should be either odom_9 or odom_10")
    sequence_id = int(opt.eval_split.split("_")[1])
    ext = getattr(opt, "ext_poses_to_eval", None)
    lines = split_lines(opt, sequence_id) if ext is None and images is None else None
    gt_path = getattr(opt, "gt_poses", None) or os.path.join(opt.data_path, "poses", "{:02d}.txt".format(sequence_id))
    if not os.path.isfile(gt_path):
        raise SystemExit("Cannot find ground-truth poses at {} (set --gt_poses)".format(gt_path))
    if ext is not None and not os.path.isfile(ext):
        raise SystemExit("Cannot find predictions at {}".format(ext))
    device = torch.device("cuda", torch.cuda.current_device())
    save_path = None
    if ext is not None:
        print("-> Loading predictions from {}".format(ext))
        pred = np.load(ext)
    else:
        folder = os.path.expanduser(opt.load_weights_folder or "")
        if not os.path.isdir(folder):
            raise SystemExit("Cannot find a folder at {}".format(folder))
        print("-> Loading weights from {}".format(folder))
        pose_encoder, pose_decoder = load_networks(folder, opt.num_layers, device)
        print("-> Computing pose predictions")
        if images is not None:
            pred = predict_poses(pose_encoder, pose_decoder, images.to(device))
        else:
            pred = predict_from_disk(pose_encoder, pose_decoder, opt, lines, device)
        save_path = os.path.join(folder, "poses.npy")
    res = evaluate_poses(pred, load_gt_poses(gt_path), TRACK_LENGTH, device)
    print(format_results(res))
    if save_path is not None:
        np.save(save_path, pred.cpu().numpy())
        print("-> Predictions saved to", save_path)
    return res


if __name__ == "__main__":
    evaluate(MonodepthOptions().parse())
