"""KITTI depth evaluation (the reference's evaluate_depth.py) on the device.

    python -m monodepth2_amd.evaluate_depth --eval_mono --ext_disp_to_eval disps.npy \\
        --gt_depths splits/eigen/gt_depths.npz

`evaluate(opt)` consumes the reference's evaluation flags (options.py): --eval_mono /
--eval_stereo, --disable_median_scaling, --pred_depth_scale_factor, --ext_disp_to_eval,
--eval_split, --post_process, --save_pred_disps, --no_eval, plus --gt_depths, the path of
the ground-truth `.npz` (key `data`; default: splits/<eval_split>/gt_depths.npz beside this
package, where the reference keeps it).  The per-image loop of evaluate_depth.py:181-214
(resize, mask, two medians, clamp, seven reductions, in numpy on the CPU) runs as the fused
HIP operator of `eval_ops.depth_metrics`, one call per group of equally sized
ground-truth maps, and prints the reference's result table.

The ground-truth file comes from `python -m monodepth2_amd.export_gt_depth` (velodyne
scans projected by csrc/velo.hip); `evaluate_from_velodyne` skips the file and evaluates
against maps projected on the device.

Out of scope here, refused with a clear error instead of half-working: loading KITTI
images from --data_path (this tree decodes no JPEGs, so predictions come from
--ext_disp_to_eval, or from `predict_disparities` on images the caller loaded), the
`benchmark` split's 16-bit PNG export (no cv2), and --eval_eigen_to_benchmark (needs the
reference's id table).  Images for `predict_disparities` are (N,3,H,W) in [0,1].
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import networks
from .eval_ops import COUNT, RATIO, depth_metrics
from .options import MonodepthOptions

STEREO_SCALE_FACTOR = 5.4   # evaluate_depth.py:21-24: 0.1-unit nominal baseline vs KITTI's 54 cm
SPLITS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "splits")


def predict_disparities(encoder, depth_decoder, images: torch.Tensor, post_process: bool = False,
                        batch_size: int = 16):
    """The raw scale-0 sigmoid disparities of `images` (N,3,H,W), evaluate_depth.py:106-123:
    eval mode, no_grad, 16 images per pass.  With `post_process` the flipped copies go
    through the network in the same batch (evaluate_depth.py:110-112) and the result is the
    pair (disp, disp_flipped), both (N,1,h,w), the second as the network produced it (not
    flipped back: depth_metrics reads it mirrored).  Fused ops that decline eval mode or
    no_grad (training-mode BatchNorm, the backward-only paths) fall back to their modules
    on their own; nothing is forced.  The modules' training flags are restored."""
    was = encoder.training, depth_decoder.training
    encoder.eval()
    depth_decoder.eval()
    disps, flipped = [], []
    try:
        with torch.no_grad():
            for i in range(0, images.shape[0], batch_size):
                x = images[i:i + batch_size]
                n = x.shape[0]
                if post_process:
                    x = torch.cat((x, torch.flip(x, [3])), 0)
                d = depth_decoder(encoder(x.contiguous()))[("disp", 0)].float()
                disps.append(d[:n].contiguous())
                if post_process:
                    flipped.append(d[n:].contiguous())
    finally:
        encoder.train(was[0])
        depth_decoder.train(was[1])
    disp = torch.cat(disps)
    return (disp, torch.cat(flipped)) if post_process else disp


def post_process_disparity(l_disp: torch.Tensor, r_disp: torch.Tensor) -> torch.Tensor:
    """batch_post_process_disparity (evaluate_depth.py:48-56) in torch, r_disp already flipped
    back; only --save_pred_disps uses it (the metrics kernel fuses the same formula)."""
    w = l_disp.shape[-1]
    l = torch.linspace(0, 1, w, device=l_disp.device, dtype=torch.float64)
    l_mask = 1.0 - torch.clamp(20 * (l - 0.05), 0, 1)
    r_mask = torch.flip(l_mask, [0])
    out = r_mask * l_disp + l_mask * r_disp + (1.0 - l_mask - r_mask) * (0.5 * (l_disp + r_disp))
    return out.to(l_disp.dtype)


def evaluate_disparities(pred_disps, gt_depths: Sequence, opt, pred_disps_flipped=None,
                         device=None, scaled: bool = False) -> Dict[str, object]:
    """evaluate_depth.py:170-221 on raw sigmoid disparities (N,h,w) or (N,1,h,w) (numpy or
    torch) against N ground-truth maps (host arrays, possibly of different sizes; or maps
    already on the device, as a (N,GH,GW) tensor or a list of device tensors, which are
    then neither stacked on the host nor uploaded).  `scaled`:
    the disparities already went through disp_to_depth (what the reference's
    --save_pred_disps files hold).  Images are
    grouped by ground-truth shape, each group is one depth_metrics call; one device-to-host
    copy at the end.  Returns {"mean_errors": (7,), "errors": (N,7), "ratios": (N,) or
    None, "ratio_median", "ratio_std", "counts": (N,)}."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    n = len(pred_disps)
    if len(gt_depths) != n:
        raise ValueError(f"{n} predictions but {len(gt_depths)} ground-truth maps")
    stereo = bool(getattr(opt, "eval_stereo", False))
    median_scaling = not (stereo or getattr(opt, "disable_median_scaling", False))
    scale_factor = STEREO_SCALE_FACTOR if stereo else float(getattr(opt, "pred_depth_scale_factor", 1))
    eigen = getattr(opt, "eval_split", "eigen") == "eigen"
    # scaled input: min_depth 1, max_depth inf make the kernel's disp_to_depth the identity
    min_depth, max_depth = (1.0, float("inf")) if scaled else (opt.min_depth, opt.max_depth)

    def to_dev(a):
        t = torch.as_tensor(a) if not torch.is_tensor(a) else a
        t = t.to(device=device, dtype=torch.float32)
        return t.unsqueeze(1) if t.dim() == 3 else t

    disp = to_dev(pred_disps)
    flipped = to_dev(pred_disps_flipped) if pred_disps_flipped is not None else None
    # ground truth born on the device (kitti_utils.generate_depth_maps) stays there: a
    # (N,GH,GW) tensor is one group as it is, device maps of a list are stacked on the device
    whole = torch.is_tensor(gt_depths) and gt_depths.is_cuda and gt_depths.dim() == 3
    groups: Dict[tuple, List[int]] = {}
    if whole:
        groups[tuple(gt_depths.shape[1:])] = list(range(n))
    else:
        for i, g in enumerate(gt_depths):
            groups.setdefault(tuple(g.shape[:2]), []).append(i)
    results = torch.empty((n, 10), dtype=torch.float32, device=device)

    def gt_of(idx):
        if whole:
            return gt_depths.to(device=device, dtype=torch.float32)
        if all(torch.is_tensor(gt_depths[i]) and gt_depths[i].is_cuda for i in idx):
            return torch.stack([gt_depths[i] for i in idx]).to(device=device, dtype=torch.float32)
        return torch.stack([torch.as_tensor(np.asarray(gt_depths[i], dtype=np.float32)) for i in idx]).to(device)

    for shape, idx in groups.items():
        sel = torch.as_tensor(idx, device=device)
        gt = gt_of(idx)
        out = depth_metrics(disp[sel], gt, mode="evaluate",
                            post_process_disp=flipped[sel] if flipped is not None else None,
                            median_scaling=median_scaling, scale_factor=scale_factor,
                            crop="eigen" if eigen else None, gt_range=eigen,
                            min_depth=min_depth, max_depth=max_depth)
        results[sel] = out
    res = results.cpu().numpy().astype(np.float64)   # the one synchronisation
    errors = res[:, :7]
    out = {"errors": errors, "mean_errors": errors.mean(0), "counts": res[:, COUNT], "ratios": None,
           "ratio_median": None, "ratio_std": None}
    if median_scaling:
        ratios = res[:, RATIO]
        med = np.median(ratios)
        out.update(ratios=ratios, ratio_median=med, ratio_std=np.std(ratios / med))
    return out


def evaluate_from_velodyne(pred_disps, frames, opt, pred_disps_flipped=None, device=None, scaled: bool = False,
                           cam: int = 2, vel_depth: bool = True) -> Dict[str, object]:
    """`evaluate_disparities` against ground truth projected here from the velodyne scans
    `frames`, a sequence of (calib_dir, velo_filename): kitti_utils.generate_depth_maps
    (csrc/velo.hip) leaves the maps on the device and depth_metrics reads them there.  The
    defaults are export_gt_depth.py's (camera 2, the points' own forward distance)."""
    from .kitti_utils import generate_depth_maps
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    gt = generate_depth_maps(frames, cam=cam, vel_depth=vel_depth, device=device)
    return evaluate_disparities(pred_disps, gt, opt, pred_disps_flipped, device, scaled=scaled)


def format_results(res) -> str:
    """The reference's table (evaluate_depth.py:216-224)."""
    lines = []
    if res["ratios"] is not None:
        lines.append(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(res["ratio_median"], res["ratio_std"]))
    lines.append("\n  " + ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"))
    lines.append(("&{: 8.3f}  " * 7).format(*res["mean_errors"].tolist()) + "\\\\")
    return "\n".join(lines)


def load_networks(folder: str, num_layers: int, device):
    """encoder.pth / depth.pth of a checkpoint folder (evaluate_depth.py:78-99)."""
    enc_dict = torch.load(os.path.join(folder, "encoder.pth"), map_location=device, weights_only=True)
    encoder = networks.ResnetEncoder(num_layers, False)
    depth_decoder = networks.DepthDecoder(encoder.num_ch_enc)
    model_dict = encoder.state_dict()
    encoder.load_state_dict({k: v for k, v in enc_dict.items() if k in model_dict}, strict=False)
    depth_decoder.load_state_dict(torch.load(os.path.join(folder, "depth.pth"), map_location=device,
                                             weights_only=True), strict=False)
    return encoder.to(device), depth_decoder.to(device)


def evaluate(opt, images: torch.Tensor = None):
    """evaluate_depth.py:59-225.  Predictions come from --ext_disp_to_eval (a .npy of
    scaled, already post-processed disparities (N,h,w): what --save_pred_disps writes, here
    and in the reference), or from `images` and the checkpoint in --load_weights_folder."""
    if sum((bool(opt.eval_mono), bool(opt.eval_stereo))) != 1:
        raise SystemExit("Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo")
    if opt.eval_eigen_to_benchmark:
        raise NotImplementedError("--eval_eigen_to_benchmark needs the reference's eigen_to_benchmark_ids.npy "
                                  "table, which this tree does not ship")
    if opt.eval_split == "benchmark" and not opt.no_eval:
        raise NotImplementedError("the `benchmark` split exports 16-bit PNGs through cv2, which this build does "
                                  "not have; use --save_pred_disps --no_eval and export them elsewhere")
    if opt.ext_disp_to_eval is None and images is None:
        raise NotImplementedError("loading KITTI frames from --data_path is out of scope (no dataset readers "
                                  "in this tree): pass --ext_disp_to_eval, or call evaluate(opt, images)")
    device = torch.device("cuda", torch.cuda.current_device())
    flipped, scaled = None, False
    if opt.ext_disp_to_eval is not None:
        print("-> Loading predictions from {}".format(opt.ext_disp_to_eval))
        pred, scaled = np.load(opt.ext_disp_to_eval), True
    else:
        folder = os.path.expanduser(opt.load_weights_folder or "")
        if not os.path.isdir(folder):
            raise SystemExit("Cannot find a folder at {}".format(folder))
        print("-> Loading weights from {}".format(folder))
        encoder, depth_decoder = load_networks(folder, opt.num_layers, device)
        print("-> Computing predictions with size {}x{}".format(images.shape[3], images.shape[2]))
        pred = predict_disparities(encoder, depth_decoder, images.to(device), opt.post_process)
        if opt.post_process:
            pred, flipped = pred
    if opt.save_pred_disps:
        out_dir = os.path.expanduser(opt.eval_out_dir or opt.load_weights_folder or ".")
        path = os.path.join(out_dir, "disps_{}_split.npy".format(opt.eval_split))
        print("-> Saving predicted disparities to ", path)
        if scaled:
            np.save(path, np.asarray(pred))
        else:
            lo, hi = 1.0 / opt.max_depth, 1.0 / opt.min_depth
            sd = lo + (hi - lo) * pred[:, 0]
            if flipped is not None:
                sd = post_process_disparity(sd, torch.flip(lo + (hi - lo) * flipped[:, 0], [2]))
            np.save(path, sd.cpu().numpy())
    if opt.no_eval:
        print("-> Evaluation disabled. Done.")
        return None
    gt_path = getattr(opt, "gt_depths", None) or os.path.join(SPLITS_DIR, opt.eval_split, "gt_depths.npz")
    if not os.path.isfile(gt_path):
        raise SystemExit("Cannot find ground truth at {} (set --gt_depths)".format(gt_path))
    gt_depths = np.load(gt_path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
    print("-> Evaluating")
    if opt.eval_stereo:
        print("   Stereo evaluation - disabling median scaling, scaling by {}".format(STEREO_SCALE_FACTOR))
    else:
        print("   Mono evaluation - using median scaling")
    res = evaluate_disparities(pred, list(gt_depths), opt, flipped, device, scaled=scaled)
    print(format_results(res))
    print("\n-> Done!")
    return res


if __name__ == "__main__":
    evaluate(MonodepthOptions().parse())
