"""GPU tests of the fused depth-evaluation operator (csrc/eval.hip, eval_ops.depth_metrics),
of evaluate_depth.predict_disparities / evaluate_disparities and of Trainer.val_step.

Yardstick: tests/eval_case.py, a numpy restatement of evaluate_depth.py:181-214 and of
Trainer.compute_depth_losses, run in fp64 (the truth) and in fp32 (the reference's own
precision); for the monitor mode also Trainer.compute_depth_losses itself.

Bars.  Thresholds: the inputs' ground truth is zeroed where the fp64 threshold ratio lies
within 1e-4 of 1.25^k (fewer than 1 % of the valid pixels), so a1, a2, a3 and the count
must match the fp64 run exactly.  Continuous metrics and the ratio: the relative error
against fp64 must not exceed 3x the fp32 formulation's own relative error against fp64
(computed here, per value), floored at 1e-7 — about one fp32 ulp, the resolution of the
fp32 outputs — so that a lucky zero floor cannot make the bar zero.  The factor 3 is the
project's usual margin over a floor.  Every figure is printed before it is asserted.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import eval_case as ec
from monodepth2_amd.eval_ops import depth_metrics

pytestmark = pytest.mark.gpu

DEV = "cuda"
CONT = (0, 1, 2, 3, 7)   # abs_rel, sq_rel, rmse, rmse_log, ratio
EXACT = (4, 5, 6, 8)     # a1, a2, a3, count


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_bar(got, e64, floor_run, what, cols=CONT):
    """got (P,>=9) vs the fp64 rows, bar = max(3 x |floor_run - e64|, 1e-7), relative."""
    got, e64, floor_run = (np.asarray(a, dtype=np.float64) for a in (got, e64, floor_run))
    worst = 0.0
    for p in range(e64.shape[0]):
        for c in cols:
            ref = e64[p, c]
            err, floor = abs(got[p, c] - ref) / abs(ref), abs(floor_run[p, c] - ref) / abs(ref)
            bar = max(3 * floor, 1e-7)
            print(f"{what} pop {p} col {c}: err {err:.3e} floor {floor:.3e} bar {bar:.3e} err/floor "
                  f"{err / max(floor, 1e-30):.2f}")
            worst = max(worst, err / bar)
    assert worst <= 1.0, (what, worst)


def check_exact(got, e64, what):
    got = np.asarray(got, dtype=np.float64)
    for c in EXACT:
        want = e64[:, c].astype(np.float32).astype(np.float64)
        print(f"{what} col {c}: got {got[:, c]} want {want}")
        assert np.array_equal(got[:, c], want), (what, c)


CONFIGS = {
    "evaluate": dict(),
    "evaluate_post_process": dict(pp=True),
    "evaluate_stereo": dict(median_scaling=False, scale_factor=5.4),
    "evaluate_no_crop": dict(crop=None),
    "evaluate_lower_median": dict(median_lower=True),
    "evaluate_pooled": dict(pool_batch=True),
    "monitor": dict(mode="monitor"),
    "monitor_per_image_np_median": dict(mode="monitor", pool_batch=False, median_lower=False),
    "monitor_post_process": dict(mode="monitor", pp=True),
    "evaluate_small_gt": dict(gt_shape=(13, 41)),
    "monitor_small_gt": dict(mode="monitor", gt_shape=(13, 41), crop=None),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the fp64 and fp32 numpy runs of a configuration (computed once)."""
    cfg = dict(CONFIGS[name])
    GH, GW = cfg.pop("gt_shape", (37, 124))
    pp = cfg.pop("pp", False)
    sig, sigf, gt = ec.make_inputs(B=3, h=24, w=80, GH=GH, GW=GW, seed=7)
    if pp:
        cfg["sig_flipped"] = sigf
    gt, removed, before = ec.clear_thresholds(sig, gt, **cfg)
    e64 = ec.evaluate_np(sig, gt, np.float64, **cfg)
    e32 = ec.evaluate_np(sig, gt, np.float32, **cfg)
    return sig, sigf if pp else None, gt, cfg, e64, e32, removed, before


def run_kernel(sig, sigf, gt, cfg, **extra):
    kw = {k: v for k, v in cfg.items() if k != "sig_flipped"}
    kw.update(extra)
    return depth_metrics(cuda(sig), cuda(gt), post_process_disp=cuda(sigf) if sigf is not None else None, **kw)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_metrics_match_the_fp64_restatement(name):
    sig, sigf, gt, cfg, e64, e32, removed, before = case(name)
    print(f"{name}: removed {removed} of {before} valid pixels near a threshold")
    assert removed < 0.01 * before
    out = run_kernel(sig, sigf, gt, cfg).cpu().numpy()
    assert out.shape == (e64.shape[0], 10) and (out[:, 9] == 0).all()
    check_exact(out, e64, name)
    check_bar(out, e64, e32, name)


@pytest.mark.parametrize("min_depth,max_depth", [(0.1, 100.0), (0.3, 70.0)])
def test_resize_agrees_with_f_interpolate(min_depth, max_depth):
    """The evaluate mode is defined as half-pixel bilinear: its prediction against
    1 / F.interpolate(scaled disparity, align_corners=False) in fp64 on the CPU, at fp32
    rounding (the kernel rounds an fp64 result once: half an ulp).  The scaled disparity is
    torch's fp32 disp_to_depth, also for depths whose reciprocals are no fp32 numbers."""
    sig, _, gt, cfg, *_ = case("evaluate_no_crop")
    _, pred, valid = depth_metrics(cuda(sig), cuda(gt), return_pred=True, min_depth=min_depth,
                                   max_depth=max_depth, **cfg)
    from monodepth2_amd.layers import disp_to_depth
    scaled = disp_to_depth(torch.from_numpy(sig), min_depth, max_depth)[0]
    assert np.array_equal(scaled.numpy(), ec.scaled_disp(sig, min_depth, max_depth))
    sd = scaled.double()
    ref = 1.0 / torch.nn.functional.interpolate(sd, gt.shape[-2:], mode="bilinear", align_corners=False)[:, 0]
    valid = valid.cpu()
    assert torch.equal(valid, torch.from_numpy(gt > 0))
    rel = ((pred.cpu().double() - ref).abs() / ref)[valid].max().item()
    print("prediction vs F.interpolate fp64, max relative:", rel)
    assert rel <= 2.0 ** -24 * 1.01


def median_inputs():
    """Four populations: odd count, even count, even count with five equal ground-truth
    values straddling the middle, one valid pixel."""
    sig, _, gt = ec.make_inputs(B=4, h=24, w=80, GH=37, GW=124, seed=19)
    for b, parity in ((0, 1), (1, 0), (2, 0)):
        idx = np.flatnonzero(gt[b])
        if idx.size % 2 != parity:
            gt[b].reshape(-1)[idx[0]] = 0
    flat = gt[2].reshape(-1)
    idx = np.flatnonzero(flat)
    order = idx[np.argsort(flat[idx])]
    mid = order.size // 2
    flat[order[mid - 3:mid + 2]] = flat[order[mid]]
    one = np.flatnonzero(gt[3])
    gt[3].reshape(-1)[one[1:]] = 0
    counts = [np.count_nonzero(g) for g in gt]
    assert counts[0] % 2 == 1 and counts[1] % 2 == 0 and counts[2] % 2 == 0 and counts[3] == 1
    return sig, gt


@pytest.mark.parametrize("lower", [False, True], ids=["np_median", "torch_median"])
def test_median_is_the_exact_order_statistic(lower):
    sig, gt = median_inputs()
    cfg = dict(crop=None, median_lower=lower)
    out, pred, valid = depth_metrics(cuda(sig), cuda(gt), return_pred=True, **cfg)
    out, pred, valid = out.cpu().numpy(), pred.cpu(), valid.cpu()
    e64 = ec.evaluate_np(sig, gt, np.float64, **cfg)
    e32 = ec.evaluate_np(sig, gt, np.float32, **cfg)
    for b in range(4):
        g, p = torch.from_numpy(gt[b])[valid[b]], pred[b][valid[b]]
        assert g.numel() == e64[b, 8] == out[b, 8]
        if lower:
            mg, mp = torch.median(g).numpy(), torch.median(p).numpy()
            assert mg == np.sort(g.numpy())[(g.numel() - 1) // 2]
        else:
            mg, mp = np.median(g.numpy()), np.median(p.numpy())
        assert mg.dtype == np.float32 and mp.dtype == np.float32
        want = np.float32(mg) / np.float32(mp)
        print(f"population {b}: n {g.numel()} median gt {mg} pred {mp} ratio {out[b, 7]!r} want {want!r}")
        assert out[b, 7] == want
    check_bar(out, e64, e32, "median", cols=(7,))


def test_gt_range_and_empty_population():
    """Four populations: ground truth 85.0 and 5e-4 inside the crop (counted only without
    the range mask), nothing valid, one valid pixel, an ordinary image.  Inclusion is
    checked on the counts and thresholds, which are exact.  The continuous bar is checked
    where the population is ordinary: the fourth image in both runs, the first under the
    range mask.  Without it the 5e-4 pixel alone is ~2000x all other terms of the first
    image's sq_rel, which is then one pixel's rounding and no statement about a reduction."""
    sig, _, gt = ec.make_inputs(B=3, h=24, w=80, GH=37, GW=124, seed=23)
    sig3, _, gt3 = ec.make_inputs(B=1, h=24, w=80, GH=37, GW=124, seed=29)
    sig, gt = np.concatenate([sig, sig3]), np.concatenate([gt, gt3])
    y0, y1, x0, x1 = ec.eigen_crop(37, 124)
    gt[0, y0 + 2, x0 + 3] = 85.0
    gt[0, y0 + 3, x0 + 5] = 5e-4
    gt[1] = 0                      # nothing valid
    gt[2, :y0] = 7.0               # valid values, all outside the crop ...
    gt[2, y0:] = 0                 # ... and none inside
    gt[2, y0 + 1, x0 + 1] = 4.0    # except one pixel
    res = {}
    for rng_on in (True, False):
        cfg = dict(gt_range=rng_on)
        g, removed, before = ec.clear_thresholds(sig, gt, **cfg)
        assert removed < 0.01 * before
        assert g[0, y0 + 2, x0 + 3] == 85.0 and g[0, y0 + 3, x0 + 5] == np.float32(5e-4)
        out = depth_metrics(cuda(sig), cuda(g), **cfg).cpu().numpy()
        e64, e32 = ec.evaluate_np(sig, g, np.float64, **cfg), ec.evaluate_np(sig, g, np.float32, **cfg)
        print("gt_range", rng_on, "counts", out[:, 8])
        assert out[1, 8] == 0 and np.isnan(out[1, :8]).all()
        assert out[2, 8] == 1 and np.isfinite(out[2, :8]).all()
        assert np.isfinite(out[[0, 3], :8]).all()
        check_exact(out[[0, 2, 3]], e64[[0, 2, 3]], f"gt_range {rng_on}")
        ordinary = [0, 3] if rng_on else [3]
        check_bar(out[ordinary], e64[ordinary], e32[ordinary], f"gt_range {rng_on}")
        res[rng_on] = (out[0, 8], np.count_nonzero(g[0, y0:y1, x0:x1]))
    # 85.0 and 5e-4 count only without the range mask
    assert res[False][0] == res[False][1] and res[True][0] == res[True][1] - 2


def test_post_process_is_the_identity_where_both_masks_vanish():
    """d_flipped = flip(d): r*d + l*d + (1-l-r)*0.5*(d+d) = d exactly where l = r = 0, so a
    crop over ground-truth columns that read only such network columns gives the plain
    result bit for bit."""
    sig, _, gt, cfg, *_ = case("evaluate_no_crop")
    w, GW, GH = sig.shape[-1], gt.shape[-1], gt.shape[-2]
    free = ec.pp_free_columns(w)
    xs = np.maximum((np.arange(GW) + 0.5) * (w / GW) - 0.5, 0)
    xa = np.minimum(np.floor(xs).astype(int), w - 1)
    ok = np.flatnonzero(free[xa] & free[np.minimum(xa + 1, w - 1)])
    x0, x1 = int(ok.min()), int(ok.max()) + 1
    assert np.array_equal(ok, np.arange(x0, x1)) and x1 - x0 > GW // 2
    crop = (0, GH, x0, x1)
    plain = depth_metrics(cuda(sig), cuda(gt), crop=crop, gt_range=False)
    flipped = np.ascontiguousarray(sig[:, :, :, ::-1])
    pp = depth_metrics(cuda(sig), cuda(gt), crop=crop, gt_range=False, post_process_disp=cuda(flipped))
    assert (plain[:, 8] > 100).all()
    assert torch.equal(plain, pp)
    # ... and not elsewhere, with a flipped pass that differs: the post-processing is live
    other = depth_metrics(cuda(sig), cuda(gt), crop=None, gt_range=False, post_process_disp=cuda(sig))
    assert not torch.equal(other, depth_metrics(cuda(sig), cuda(gt), crop=None, gt_range=False))


@pytest.mark.parametrize("name", ["evaluate_post_process", "monitor"])
def test_bitwise_repeatable_and_capturable(name):
    sig, sigf, gt, cfg, *_ = case(name)
    kw = {k: v for k, v in cfg.items() if k != "sig_flipped"}
    d, g = cuda(sig), cuda(gt)
    f = cuda(sigf) if sigf is not None else None
    a = depth_metrics(d, g, post_process_disp=f, **kw)
    b = depth_metrics(d, g, post_process_disp=f, **kw)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        depth_metrics(d, g, post_process_disp=f, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = depth_metrics(d, g, post_process_disp=f, **kw)
    replays = []
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        replays.append(out.clone())
    torch.cuda.synchronize()
    for r in replays:
        assert torch.equal(r.view(torch.int32), a.view(torch.int32))


def test_kernel_reproduces_the_reference_golden():
    """tests/golden/depth_eval/depth_eval_monitor.npz: the reference's own compute_depth_losses (fp32,
    CPU) at 375 x 1242.  The kernel against the fp64 restatement, with the golden — the
    fp32 reference formulation itself — as the floor."""
    sig, gt, golden = ec.load_golden()
    e64 = ec.evaluate_np(sig, gt, np.float64, mode="monitor")
    out = depth_metrics(cuda(sig), cuda(gt), mode="monitor").cpu().numpy()
    floor = np.concatenate([golden, [np.nan, np.nan]])[None]
    check_exact(out, e64, "golden")
    check_bar(out, e64, floor, "golden", cols=(0, 1, 2, 3))
    assert np.abs(out[0, 4:7] - golden[4:7]).max() < 2.4e-7   # fp32 means of the same counts


# ------------------------------------------------------------------ networks

def small_networks():
    from monodepth2_amd import networks
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False)
    dec = networks.DepthDecoder(enc.num_ch_enc)
    return enc, dec


def test_predict_disparities_no_worse_than_stock_modules(monkeypatch):
    from monodepth2_amd import bn_ops, conv_ops, stem_ops
    from monodepth2_amd.evaluate_depth import predict_disparities
    enc, dec = small_networks()
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, 64, 128, generator=g)
    with torch.no_grad():
        e64, d64 = copy.deepcopy(enc).double().eval(), copy.deepcopy(dec).double().eval()
        exact = d64(e64(images.double()))[("disp", 0)]
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV).to(memory_format=torch.channels_last)
    enc.train()
    ours = predict_disparities(enc, dec, images.to(DEV))
    assert enc.training and dec.training               # flags restored
    assert ours.shape == (2, 1, 64, 128) and ours.dtype == torch.float32
    for mod in (bn_ops, conv_ops, stem_ops):           # stock: every fused path off
        monkeypatch.setattr(mod, "ENABLED", False)
    monkeypatch.setattr(stem_ops, "FWD_ENABLED", False)
    stock_dec = copy.deepcopy(dec)
    stock_dec.fused = False
    enc.eval(), stock_dec.eval()
    with torch.no_grad():
        ref = stock_dec(enc(images.to(DEV)))[("disp", 0)]
    e_ours = (ours.cpu().double() - exact).abs().max().item()
    e_ref = (ref.cpu().double() - exact).abs().max().item()
    print("predict_disparities: e_ours", e_ours, "e_ref (stock fp32 modules)", e_ref)
    assert e_ours <= 3 * e_ref


def test_post_process_prediction_bookkeeping():
    """predict_disparities(post_process=True): the flipped copies ride in the same batch;
    the second result is the network's output for the flipped image, not flipped back, and
    evaluate_disparities hands both to the kernel — checked against the restatement that
    flips it back itself.  Two ground-truth sizes exercise the grouping by shape."""
    from monodepth2_amd.evaluate_depth import evaluate_disparities, predict_disparities
    from monodepth2_amd.options import default_options
    enc, dec = small_networks()
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    images = torch.rand(3, 3, 64, 128, generator=g).to(DEV)
    disp, flipped = predict_disparities(enc, dec, images, post_process=True)
    assert disp.shape == flipped.shape == (3, 1, 64, 128)
    plain = predict_disparities(enc, dec, images)
    of_flipped = predict_disparities(enc, dec, torch.flip(images, [3]))
    assert torch.allclose(disp, plain, atol=1e-5) and torch.allclose(flipped, of_flipped, atol=1e-5)
    assert not torch.allclose(flipped, disp, atol=1e-5)
    sig, sigf = disp.cpu().numpy(), flipped.cpu().numpy()
    rng = np.random.default_rng(5)
    shapes = [(37, 124), (13, 41), (37, 124)]
    gts, e64, e32 = [], [], []
    for i, (GH, GW) in enumerate(shapes):
        cfg = dict(sig_flipped=sigf[i:i + 1])
        gt = ec.gt_around(sig[i:i + 1], GH, GW, rng)
        gt, removed, before = ec.clear_thresholds(sig[i:i + 1], gt, **cfg)
        assert removed < 0.01 * before
        gts.append(gt[0])
        e64.append(ec.evaluate_np(sig[i:i + 1], gt, np.float64, **cfg)[0])
        e32.append(ec.evaluate_np(sig[i:i + 1], gt, np.float32, **cfg)[0])
    e64, e32 = np.array(e64), np.array(e32)
    res = evaluate_disparities(disp, gts, default_options(eval_mono=True, post_process=True), flipped)
    got = np.concatenate([res["errors"], res["ratios"][:, None], res["counts"][:, None]], 1)
    check_exact(got, e64, "evaluate_disparities")
    check_bar(got, e64, e32, "evaluate_disparities")
    assert np.allclose(res["mean_errors"], res["errors"].mean(0))
    # stereo: scale factor 5.4, no median scaling (evaluate_depth.py:170-174)
    stereo = evaluate_disparities(disp, gts, default_options(eval_stereo=True), None)
    assert stereo["ratios"] is None
    s64, s32 = (np.array([ec.evaluate_np(sig[i:i + 1], gts[i][None], dt, median_scaling=False,
                                         scale_factor=5.4)[0] for i in range(3)]) for dt in (np.float64, np.float32))
    check_bar(stereo["errors"], s64, s32, "evaluate_disparities stereo", cols=(0, 1, 2, 3))


def test_evaluate_from_npy_files(tmp_path, capsys):
    """evaluate(opt) as `python -m monodepth2_amd.evaluate_depth` runs it: scaled disparities
    from --ext_disp_to_eval (the reference's file format), ground truth from --gt_depths,
    the reference's table on stdout, --save_pred_disps writing the same array back."""
    from monodepth2_amd.evaluate_depth import evaluate
    from monodepth2_amd.options import MonodepthOptions
    sig, _, gt, cfg, e64, e32, *_ = case("evaluate")
    np.save(tmp_path / "disps.npy", ec.scaled_disp(sig[:, 0]))
    np.savez(tmp_path / "gt_depths.npz", data=gt)
    res = evaluate(MonodepthOptions().parse(["--eval_mono", "--ext_disp_to_eval", str(tmp_path / "disps.npy"),
                                             "--gt_depths", str(tmp_path / "gt_depths.npz"), "--save_pred_disps",
                                             "--eval_out_dir", str(tmp_path)]))
    got = np.concatenate([res["errors"], res["ratios"][:, None], res["counts"][:, None]], 1)
    check_exact(got, e64, "evaluate from files")
    check_bar(got, e64, e32, "evaluate from files")
    text = capsys.readouterr().out
    assert " Scaling ratios | med: " in text and "Mono evaluation - using median scaling" in text
    assert ("{:>8} | " * 7).format("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3") in text
    assert ("&{: 8.3f}  " * 7).format(*e64[:, :7].mean(0).tolist()) + "\\\\" in text
    assert np.array_equal(np.load(tmp_path / "disps_eigen_split.npy"), ec.scaled_disp(sig[:, 0]))


@pytest.mark.parametrize("amp", ["none", "bf16"])
def test_val_step_matches_compute_depth_losses_and_keeps_training_state(amp):
    from monodepth2_amd.data import synthetic_batch
    from monodepth2_amd.options import default_options
    from monodepth2_amd.trainer import Trainer
    B, H, W = 2, 64, 128
    torch.manual_seed(0)
    tr = Trainer(default_options(batch_size=B, height=H, width=W, weights_init="scratch", log_dir="/tmp/md2_test",
                                 frame_ids=[0, -1, 1], amp=amp), device=torch.device(DEV, 0))
    batch = synthetic_batch(B, H, W, tr.opt.frame_ids, 4, seed=3, device=DEV)
    tr.set_train()
    tr.train_step(batch)   # BatchNorm statistics and step counters away from their initial values

    def state():
        return ([p.detach().clone() for p in tr.parameters_to_train],
                [b.detach().clone() for m in tr.models.values() for b in m.buffers()],
                tr._bn_steps, tr.step, [m.training for m in tr.models.values()])

    before = state()
    outputs, losses = tr.val_step(batch)           # no depth_gt: losses only
    assert "de/abs_rel" not in losses and torch.isfinite(losses["loss"])
    sig = outputs[("disp", 0)].float().cpu().numpy()
    gt = ec.gt_around(sig, 375, 1242, np.random.default_rng(9), density=0.03)
    gt, removed, n_valid = ec.clear_thresholds(sig, gt, mode="monitor")
    assert removed < 0.01 * n_valid
    batch["depth_gt"] = cuda(gt).unsqueeze(1)
    outputs, losses = tr.val_step(batch)
    after = state()
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert torch.equal(a, b)
    assert before[2:] == after[2:] and all(after[4])
    assert np.array_equal(outputs[("disp", 0)].float().cpu().numpy(), sig)
    got = torch.stack([losses[n] for n in tr.depth_metric_names]).cpu().numpy()
    assert all(losses[n].is_cuda for n in tr.depth_metric_names)
    # the eager yardstick on the same outputs
    eager = {}
    with torch.no_grad():
        tr.generate_images_pred(batch, outputs)
        tr.compute_depth_losses(batch, outputs, eager)
    eager = np.array([float(eager[n]) for n in tr.depth_metric_names])
    e64 = ec.evaluate_np(sig, gt, np.float64, mode="monitor")
    pad = [np.nan, e64[0, 8]]
    check_exact(np.concatenate([got, pad])[None], e64, "val_step")
    check_bar(np.concatenate([got, pad])[None], e64, np.concatenate([eager, pad])[None], "val_step",
              cols=(0, 1, 2, 3))
