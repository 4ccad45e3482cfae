"""KITTI depth evaluation (the reference's evaluate_depth.py) on the device.

    python -m monodepth2_amd.evaluate_depth --eval_mono --load_weights_folder W \\
        --data_path KITTI --split_dir splits/eigen --gt_depths splits/eigen/gt_depths.npz
    python -m monodepth2_amd.evaluate_depth --eval_mono --ext_disp_to_eval disps.npy \\
        --gt_depths splits/eigen/gt_depths.npz

`evaluate(opt)` consumes the reference's evaluation flags (options.py): --eval_mono /
--eval_stereo, --disable_median_scaling, --pred_depth_scale_factor, --ext_disp_to_eval,
--eval_split, --post_process, --save_pred_disps, --no_eval, --eval_eigen_to_benchmark,
--eval_out_dir, plus --gt_depths, the path of the ground-truth `.npz` (key `data`; default:
splits/<eval_split>/gt_depths.npz beside this package, where the reference keeps it),
--split_dir, the folder of the split's test_files.txt (default splits/<eval_split>/ beside
this package; the lists are not shipped), and --eigen_to_benchmark_ids, the reference's id
table for --eval_eigen_to_benchmark.  The per-image loop of evaluate_depth.py:181-214
(resize, mask, two medians, clamp, seven reductions, in numpy on the CPU) runs as the fused
HIP operator of `eval_ops.depth_metrics`, one call per group of equally sized
ground-truth maps, and prints the reference's result table.

The ground-truth file comes from `python -m monodepth2_amd.export_gt_depth` (velodyne
scans projected by csrc/velo.hip); `evaluate_from_velodyne` skips the file and evaluates
against maps projected on the device.

Predictions come from --ext_disp_to_eval, from `images` the caller loaded ((N,3,H,W) in
[0,1]), or, as in the reference, from the frames test_files.txt names under --data_path:
datasets.KITTIRAWDataset decodes them, loader.BatchLoader (list order, 16 per pass, the
partial last batch included, scale 0 only) resizes them on the device to the size
encoder.pth was trained at, bit-equal to the reference's PIL pipeline, and the raw sigmoid
disparities never leave the device before the metrics.

`--eval_split benchmark` writes the KITTI benchmark's submission files instead of
evaluating: 352 x 1216 16-bit PNGs of depth * 256 in <--eval_out_dir or
--load_weights_folder>/benchmark_predictions/, made by `eval_ops.benchmark_depth_maps` (one
HIP launch per 64 images) and written through Pillow.  The predictions then come from
--ext_disp_to_eval or `images`: the reference's splits/benchmark/test_files.txt (`image N`
lines) names nothing KITTIRAWDataset can resolve, in the reference either, so that
combination is refused.  --eval_eigen_to_benchmark applies to external predictions only, as
in the reference.

What a command line lacks is reported before anything loads: a missing split list as
`options.SplitListMissing` (a FileNotFoundError that names --split_dir), a benchmark export
without an output folder, the benchmark split from --data_path and a missing id table as
`options.EvalRefused` (a SystemExit that names the flag).  Both are NotImplementedErrors as
well: these command lines were refused with one before the routes existed, and a caller
that caught it still does.

Two runs of the networks agree to the last bit only under
`torch.backends.cudnn.deterministic = True`; by default the convolution library may choose
kernels whose sums are not ordered (one unit in the last place on some pixels).
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import networks
from .datasets import readlines
from .eval_ops import COUNT, RATIO, benchmark_depth_maps, depth_metrics, write_benchmark_pngs
from .options import EvalRefused, MonodepthOptions, SplitListMissing

STEREO_SCALE_FACTOR = 5.4   # evaluate_depth.py:21-24: 0.1-unit nominal baseline vs KITTI's 54 cm
SPLITS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "splits")
EIGEN_TO_BENCHMARK_IDS = os.path.join(SPLITS_DIR, "benchmark", "eigen_to_benchmark_ids.npy")
BENCHMARK_HW = (352, 1216)  # evaluate_depth.py:155
BENCHMARK_CHUNK = 64        # images per export launch and device-to-host copy


def _disparity_batch(encoder, depth_decoder, x: torch.Tensor, post_process: bool):
    """One pass of evaluate_depth.py:106-123 on `x` (n,3,H,W): (disp, disp_flipped or None),
    both (n,1,h,w).  The caller holds eval mode and no_grad."""
    n = x.shape[0]
    if post_process:
        x = torch.cat((x, torch.flip(x, [3])), 0)
    d = depth_decoder(encoder(x.contiguous()))[("disp", 0)].float()
    return d[:n].contiguous(), (d[n:].contiguous() if post_process else None)


def _predict_batches(encoder, depth_decoder, batches, post_process: bool):
    """`_disparity_batch` over an iterable of image batches, in eval mode under no_grad; the
    modules' training flags are restored."""
    was = encoder.training, depth_decoder.training
    encoder.eval()
    depth_decoder.eval()
    disps, flipped = [], []
    try:
        with torch.no_grad():
            for x in batches:
                d, f = _disparity_batch(encoder, depth_decoder, x, post_process)
                disps.append(d)
                if post_process:
                    flipped.append(f)
    finally:
        encoder.train(was[0])
        depth_decoder.train(was[1])
    disp = torch.cat(disps)
    return (disp, torch.cat(flipped)) if post_process else disp


def predict_disparities(encoder, depth_decoder, images: torch.Tensor, post_process: bool = False,
                        batch_size: int = 16):
    """The raw scale-0 sigmoid disparities of `images` (N,3,H,W), evaluate_depth.py:106-123:
    eval mode, no_grad, 16 images per pass.  With `post_process` the flipped copies go
    through the network in the same batch (evaluate_depth.py:110-112) and the result is the
    pair (disp, disp_flipped), both (N,1,h,w), the second as the network produced it (not
    flipped back: depth_metrics reads it mirrored).  Fused ops that decline eval mode or
    no_grad (training-mode BatchNorm, the backward-only paths) fall back to their modules
    on their own; nothing is forced.  The modules' training flags are restored."""
    return _predict_batches(encoder, depth_decoder,
                            (images[i:i + batch_size] for i in range(0, images.shape[0], batch_size)), post_process)


def split_lines(opt, split: str, name: str = "test_files.txt") -> List[str]:
    """The lines of the list `name` in --split_dir (default splits/<split>/ beside this
    package, where the reference keeps it; the lists are not shipped)."""
    path = os.path.join(getattr(opt, "split_dir", None) or os.path.join(SPLITS_DIR, split), name)
    if not os.path.isfile(path):
        raise SplitListMissing(
            "no split list at {}: evaluating the frames under --data_path needs it, and the split lists are "
            "not shipped with this package; pass --split_dir DIR with DIR/{} (the reference's splits/{}/ "
            "folder)".format(path, name, split))
    return readlines(path)


def predict_from_disk(encoder, depth_decoder, opt, lines, feed_hw, device, batch_size: int = 16):
    """evaluate_depth.py:66-123 from --data_path: the frames the split lines `lines` name,
    decoded by datasets.KITTIRAWDataset, resized to the checkpoint's feed size on the device
    (loader.BatchLoader in list order, the partial last batch included; scale 0 only), then
    the per-batch body of `predict_disparities`."""
    from .datasets import KITTIRAWDataset
    from .loader import BatchLoader
    from .pack import open_pack
    dataset = KITTIRAWDataset(opt.data_path, lines, feed_hw[0], feed_hw[1], [0], 1, is_train=False,
                              img_ext=".png" if opt.png else ".jpg")
    loader = BatchLoader(dataset, batch_size, shuffle=False, drop_last=False, num_workers=opt.num_workers,
                         device=device, device_decode=getattr(opt, "device_decode", False), pack=open_pack(opt),
                         device_png=getattr(opt, "device_png", False))
    try:
        return _predict_batches(encoder, depth_decoder, (batch[("color", 0, 0)] for batch in loader),
                                opt.post_process)
    finally:
        loader.close()


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
    """encoder.pth / depth.pth of a checkpoint folder (evaluate_depth.py:78-99) and the
    (height, width) the encoder was trained at, which encoder.pth carries beside its
    weights (None for a file without them: only the --data_path route needs the size)."""
    enc_dict = torch.load(os.path.join(folder, "encoder.pth"), map_location=device, weights_only=True)
    sized = "height" in enc_dict and "width" in enc_dict
    feed_hw = (int(enc_dict["height"]), int(enc_dict["width"])) if sized else None
    encoder = networks.ResnetEncoder(num_layers, False)
    depth_decoder = networks.DepthDecoder(encoder.num_ch_enc)
    model_dict = encoder.state_dict()
    encoder.load_state_dict({k: v for k, v in enc_dict.items() if k in model_dict}, strict=False)
    depth_decoder.load_state_dict(torch.load(os.path.join(folder, "depth.pth"), map_location=device,
                                             weights_only=True), strict=False)
    return encoder.to(device), depth_decoder.to(device), feed_hw


def export_benchmark(pred, flipped, scaled: bool, opt, save_dir: str, device, chunk: int = BENCHMARK_CHUNK):
    """evaluate_depth.py:148-163: the predictions as the benchmark's 352 x 1216 16-bit PNGs
    in `save_dir`, at most `chunk` images per launch and per device-to-host copy."""
    min_depth, max_depth = (1.0, float("inf")) if scaled else (opt.min_depth, opt.max_depth)

    def to_dev(a):
        t = torch.as_tensor(a) if not torch.is_tensor(a) else a
        return t.to(device=device, dtype=torch.float32)

    paths = []
    for i in range(0, len(pred), chunk):
        maps = benchmark_depth_maps(to_dev(pred[i:i + chunk]),
                                    to_dev(flipped[i:i + chunk]) if flipped is not None else None,
                                    out_hw=BENCHMARK_HW, scale_factor=STEREO_SCALE_FACTOR, clip_max=80.0, quant=256.0,
                                    min_depth=min_depth, max_depth=max_depth)
        paths += write_benchmark_pngs(maps, save_dir, start=i,
                                      device_encode=bool(getattr(opt, "device_png_encode", False)))
    return paths


def evaluate(opt, images: torch.Tensor = None, batch_size: int = 16):
    """evaluate_depth.py:59-225.  Predictions come from --ext_disp_to_eval (a .npy of
    scaled, already post-processed disparities (N,h,w): what --save_pred_disps writes, here
    and in the reference), or from the checkpoint in --load_weights_folder run on `images`
    (N,3,H,W) or, without them, on the frames the split's test_files.txt names under
    --data_path (`predict_from_disk`), `batch_size` images per pass.  `--eval_split
    benchmark` writes the benchmark's PNGs instead of evaluating and returns their paths."""
    if sum((bool(opt.eval_mono), bool(opt.eval_stereo))) != 1:
        raise SystemExit("Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo")
    benchmark = opt.eval_split == "benchmark"
    save_dir = None
    if benchmark and not opt.no_eval:
        if not (opt.eval_out_dir or opt.load_weights_folder):
            raise EvalRefused("the benchmark split writes its PNGs into <folder>/benchmark_predictions: set "
                             "--eval_out_dir or --load_weights_folder")
        save_dir = os.path.join(os.path.expanduser(opt.eval_out_dir or opt.load_weights_folder),
                                "benchmark_predictions")
    ids = None
    if opt.eval_eigen_to_benchmark and opt.ext_disp_to_eval is not None:   # external predictions only, as the reference
        ids_path = getattr(opt, "eigen_to_benchmark_ids", None) or EIGEN_TO_BENCHMARK_IDS
        if not os.path.isfile(ids_path):
            raise EvalRefused("Cannot find the id table at {} (set --eigen_to_benchmark_ids; the reference keeps it "
                             "at splits/benchmark/eigen_to_benchmark_ids.npy)".format(ids_path))
        ids = np.load(ids_path)
    flipped, scaled = None, False
    if opt.ext_disp_to_eval is not None:
        device = torch.device("cuda", torch.cuda.current_device())
        print("-> Loading predictions from {}".format(opt.ext_disp_to_eval))
        pred, scaled = np.load(opt.ext_disp_to_eval), True
        if ids is not None:
            pred = pred[ids]
    else:
        if images is None and benchmark:
            raise EvalRefused("the benchmark split cannot be read from --data_path: the lines of the reference's "
                             "splits/benchmark/test_files.txt (`image N`) name no KITTI raw frame, in the reference "
                             "either; pass --ext_disp_to_eval, or call evaluate(opt, images)")
        if images is None:   # a missing list is reported before anything loads
            lines = split_lines(opt, opt.eval_split)
        device = torch.device("cuda", torch.cuda.current_device())
        folder = os.path.expanduser(opt.load_weights_folder or "")
        if not os.path.isdir(folder):
            raise SystemExit("Cannot find a folder at {}".format(folder))
        print("-> Loading weights from {}".format(folder))
        encoder, depth_decoder, feed_hw = load_networks(folder, opt.num_layers, device)
        if images is not None:
            print("-> Computing predictions with size {}x{}".format(images.shape[3], images.shape[2]))
            pred = predict_disparities(encoder, depth_decoder, images.to(device), opt.post_process, batch_size)
        else:
            if feed_hw is None:
                raise SystemExit("{} carries no height / width: not an encoder.pth a training run saved".format(
                    os.path.join(folder, "encoder.pth")))
            print("-> Computing predictions with size {}x{}".format(feed_hw[1], feed_hw[0]))
            pred = predict_from_disk(encoder, depth_decoder, opt, lines, feed_hw, device, batch_size)
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
    if benchmark:
        print("-> Saving out benchmark predictions to {}".format(save_dir))
        paths = export_benchmark(pred, flipped, scaled, opt, save_dir, device)
        print("-> No ground truth is available for the KITTI benchmark, so not evaluating. Done.")
        return paths
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
