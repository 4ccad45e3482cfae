"""Shared by tests/test_eval_*.py: a numpy restatement of the reference's depth evaluation
in a chosen precision, and the synthetic inputs the tests run it on.

`evaluate_np` restates evaluate_depth.py:181-214 (mode "evaluate": resize the scaled
disparity with half-pixel bilinear weights, invert, mask, np.median scaling per image,
clamp, compute_errors 27-45) and Trainer.compute_depth_losses, trainer.py:498-526 (mode
"monitor": resize the depth, clamp, gt > 0 inside the crop, one torch.median-convention
scaling over the batch, clamp, compute_depth_errors).  `dt` is the precision of every
step after disp_to_depth, which is always torch's fp32 product and sum — the array the
reference's evaluation starts from.  dt=float64 is the yardstick, dt=float32 the fp32
formulation whose own error against it is the floor of the tests' bars.
"""
import os

import numpy as np

THRESH = (1.25, 1.25 ** 2, 1.25 ** 3)
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0


def scaled_disp(sig, min_depth=0.1, max_depth=100.0):
    """disp_to_depth's scaled disparity as torch computes it in fp32 (layers.py:16-25)."""
    lo, hi = 1.0 / max_depth, 1.0 / min_depth
    return (np.float32(lo) + (np.float32(hi - lo) * sig.astype(np.float32)).astype(np.float32)).astype(np.float32)


def resize(a, GH, GW, dt):
    """Half-pixel bilinear (F.interpolate align_corners=False) of (..., h, w) in `dt`."""
    h, w = a.shape[-2:]
    ys = (np.arange(GH, dtype=dt) + dt(0.5)) * dt(h / GH) - dt(0.5)
    xs = (np.arange(GW, dtype=dt) + dt(0.5)) * dt(w / GW) - dt(0.5)
    ys, xs = np.maximum(ys, dt(0)), np.maximum(xs, dt(0))
    y0 = np.minimum(np.floor(ys).astype(int), h - 1)
    x0 = np.minimum(np.floor(xs).astype(int), w - 1)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = (ys - y0.astype(dt))[:, None], (xs - x0.astype(dt))[None, :]
    a = a.astype(dt)
    top = a[..., y0, :][..., :, x0] * (dt(1) - fx) + a[..., y0, :][..., :, x1] * fx
    bot = a[..., y1, :][..., :, x0] * (dt(1) - fx) + a[..., y1, :][..., :, x1] * fx
    return top * (dt(1) - fy) + bot * fy


def post_process(l_disp, r_disp, dt):
    """batch_post_process_disparity (evaluate_depth.py:48-56); r_disp already flipped back."""
    w = l_disp.shape[-1]
    l = np.linspace(0, 1, w).astype(dt)
    l_mask = dt(1) - np.clip(dt(20) * (l - dt(0.05)), dt(0), dt(1))
    r_mask = l_mask[::-1]
    l_disp, r_disp = l_disp.astype(dt), r_disp.astype(dt)
    return r_mask * l_disp + l_mask * r_disp + (dt(1) - l_mask - r_mask) * (dt(0.5) * (l_disp + r_disp))


def pp_free_columns(w):
    """Network columns where both post-processing masks are exactly 0."""
    l = np.linspace(0, 1, w)
    l_mask = 1.0 - np.clip(20 * (l - 0.05), 0, 1)
    return (l_mask == 0) & (l_mask[::-1] == 0)


def eigen_crop(GH, GW):
    c = np.array([0.40810811 * GH, 0.99189189 * GH, 0.03594771 * GW, 0.96405229 * GW]).astype(np.int32)
    return tuple(int(v) for v in c)


def median(x, lower):
    """torch.median (the element at (n-1)/2) or np.median, in x's dtype."""
    if lower:
        return np.sort(x)[(x.size - 1) // 2]
    return np.median(x)


def errors(gt, pred):
    """compute_errors (evaluate_depth.py:27-45) + the per-pixel threshold ratio."""
    t = np.maximum(gt / pred, pred / gt)
    out = [np.mean(np.abs(gt - pred) / gt), np.mean((gt - pred) ** 2 / gt), np.sqrt(((gt - pred) ** 2).mean()),
           np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())] + [(t < k).mean() for k in THRESH]
    return np.array(out, dtype=np.float64), t


def predict_np(sig, gt_shape, dt, mode="evaluate", sig_flipped=None, scale_factor=1.0, min_depth=0.1,
               max_depth=100.0):
    """(B,GH,GW) depth prediction before masking and median scaling."""
    sd = scaled_disp(sig[:, 0], min_depth, max_depth)
    if sig_flipped is not None:
        sd = post_process(sd, scaled_disp(sig_flipped[:, 0], min_depth, max_depth)[:, :, ::-1], dt)
    sd = sd.astype(dt)
    GH, GW = gt_shape
    if mode == "monitor":
        pred = np.clip(resize(dt(1) / sd, GH, GW, dt), dt(MIN_DEPTH), dt(MAX_DEPTH)) * dt(scale_factor)
    else:
        pred = dt(scale_factor) / resize(sd, GH, GW, dt)
    return pred.astype(dt)


def valid_mask(gt, crop, gt_range):
    GH, GW = gt.shape[-2:]
    m = ((gt > np.float32(MIN_DEPTH)) & (gt < np.float32(MAX_DEPTH))) if gt_range else (gt > 0)
    y0, y1, x0, x1 = (0, GH, 0, GW) if crop is None else (eigen_crop(GH, GW) if crop == "eigen" else crop)
    c = np.zeros(gt.shape[-2:], bool)
    c[y0:y1, x0:x1] = True
    return m & c


def evaluate_np(sig, gt, dt, mode="evaluate", sig_flipped=None, median_scaling=True, scale_factor=1.0,
                crop="eigen", gt_range=None, pool_batch=None, median_lower=None, want_thresh=False):
    """-> (P,9) float64: the seven metrics, the ratio, the count (NaN / 0 for an empty
    population); with want_thresh also the per-population threshold ratios."""
    monitor = mode == "monitor"
    gt_range = ((not monitor) and crop == "eigen") if gt_range is None else gt_range
    pool_batch = monitor if pool_batch is None else pool_batch
    median_lower = monitor if median_lower is None else median_lower
    pred = predict_np(sig, gt.shape[-2:], dt, mode, sig_flipped, scale_factor)
    mask = valid_mask(gt, crop, gt_range)
    pops = [slice(None)] if pool_batch else [slice(i, i + 1) for i in range(gt.shape[0])]
    rows, threshes = [], []
    for sl in pops:
        m = mask[sl]
        g, p = gt[sl][m].astype(dt), pred[sl][m]
        if g.size == 0:
            rows.append([np.nan] * 8 + [0])
            threshes.append(np.zeros(0))
            continue
        ratio = dt(1)
        if median_scaling:
            ratio = median(g, median_lower) / median(p, median_lower)
            p = p * ratio
        p = np.clip(p, dt(MIN_DEPTH), dt(MAX_DEPTH))
        e, t = errors(g, p)
        rows.append(list(e) + [float(ratio), g.size])
        threshes.append(t)
    out = np.array(rows, dtype=np.float64)
    return (out, threshes) if want_thresh else out


def make_inputs(B=3, h=24, w=80, GH=37, GW=124, seed=7, density=0.25):
    """Smooth sigmoid disparities and LiDAR-like ground truth (~25 % density) scattered
    around 3x the predicted depth, so median scaling has work to do."""
    rng = np.random.default_rng(seed)
    sig = rng.uniform(0.02, 0.98, (B, 1, h + 2, w + 2))
    sig = sum(sig[:, :, i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0   # 3x3 box blur
    sig = sig.astype(np.float32)
    sigf = rng.uniform(0.02, 0.98, (B, 1, h, w)).astype(np.float32) * np.float32(0.2) + sig[:, :, :, ::-1] * np.float32(0.8)
    return sig, np.ascontiguousarray(sigf), gt_around(sig, GH, GW, rng, density)


def gt_around(sig, GH, GW, rng, density=0.25):
    """(B,GH,GW) sparse ground truth scattered (sigma 0.25 in log) around ~3x the depth the
    sigmoid disparities `sig` (B,1,h,w) predict."""
    B = sig.shape[0]
    depth = 1.0 / resize(scaled_disp(sig[:, 0]), GH, GW, np.float64)
    true = depth * rng.uniform(2.5, 3.5, (B, 1, 1)) * np.exp(rng.normal(0, 0.25, (B, GH, GW)))
    return np.where(rng.random((B, GH, GW)) < density, true, 0.0).astype(np.float32)


def clear_thresholds(sig, gt, rel=1e-4, **cfg):
    """Zero the ground truth at pixels whose fp64 threshold ratio lies within `rel` of 1.25,
    1.25^2 or 1.25^3 (an fp32 evaluation may put those on the other side), repeating because
    a removal moves the medians.  -> (gt, removed, valid_before)."""
    gt = gt.copy()
    gt_range = cfg.get("gt_range")
    mode, crop = cfg.get("mode", "evaluate"), cfg.get("crop", "eigen")
    if gt_range is None:
        gt_range = mode != "monitor" and crop == "eigen"
    pool = cfg.get("pool_batch")
    pool = (mode == "monitor") if pool is None else pool
    before = int(valid_mask(gt, crop, gt_range).sum())
    removed = 0
    for _ in range(20):
        _, threshes = evaluate_np(sig, gt, np.float64, want_thresh=True, **cfg)
        mask = valid_mask(gt, crop, gt_range)
        hit = False
        for pi, t in enumerate(threshes):
            near = np.zeros(t.shape, bool)
            for k in THRESH:
                near |= np.abs(t / k - 1) < rel
            if near.any():
                hit = True
                sl = slice(None) if pool else slice(pi, pi + 1)
                idx = np.argwhere(mask[sl])[near]
                sub = gt[sl]
                sub[idx[:, 0], idx[:, 1], idx[:, 2]] = 0
                removed += int(near.sum())
        if not hit:
            return gt, removed, before
    raise AssertionError("threshold clearing did not settle")


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_eval",
                      "depth_eval_monitor.npz")


def load_golden():
    """tests/golden/depth_eval/depth_eval_monitor.npz (make_depth_eval_golden.py beside it) -> sig (2,1,24,80),
    gt (2,375,1242) rebuilt from its sparse form, the reference's seven fp32 metrics."""
    z = np.load(GOLDEN)
    gt = np.zeros(int(np.prod(z["gt_shape"])), np.float32)
    gt[z["gt_index"]] = z["gt_value"]
    return z["sig"], gt.reshape(tuple(z["gt_shape"])), z["metrics"].astype(np.float64)
