"""md2_log_panel on the GPU against the numpy restatement (tests/logpanel_case.py), the
recorded results of the reference's normalize_image, md2_generate_images (bitwise) and the
reference's own warps (tests/golden/logpanel/)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_io import Case
from hotpath_case import case_config, case_operands
from monodepth2_amd import _lib
from monodepth2_amd.data import synthetic_batch, synthetic_hotpath
from monodepth2_amd.hotpath import (HotPathConfig, generate_images, photometric_loss, predictive_mask_inputs,
                                    selection_maps)
from monodepth2_amd.layers import transformation_from_parameters
from monodepth2_amd.log_ops import log_panel, panel_layout, run_tiles

import logpanel_case as lc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "logpanel")
DEV = "cuda"


def single(kind, a, dtype=torch.float32, prefill=None):
    """One tile of `kind` holding `a` ((3,h,w) or (h,w)) alone on an h x up4(w) sheet."""
    a = np.asarray(a, np.float32)
    h, w = a.shape[-2:]
    cfg = HotPathConfig(batch=1, height=h, width=w, num_src=1, num_scales=1)
    disp = torch.from_numpy(a if a.ndim == 2 else np.zeros((h, w), np.float32)).to(DEV, dtype).view(1, 1, h, w)
    src = disp[0] if kind == lc.DISP else torch.from_numpy(a).to(DEV)
    SW = (w + 3) // 4 * 4
    panel = run_tiles(cfg, 1, (h, SW), {"t/0": (0, 0, h, w)}, [(kind, 0, 0, 0, (0, 0, h, w), src)], [disp])
    torch.cuda.synchronize()
    return panel, lc.build_sheet(1, h, SW, [(kind, 0, (0, 0, h, w), a)])


def test_quantise_dword_and_tail_paths():
    probe = lc.quantise_probe()                       # 773 values
    a = np.full(3 * 8 * 40, 0.5, np.float32)
    a[:probe.size] = probe
    a = a.reshape(3, 8, 40)
    panel, want = single(lc.COLOR, a)
    got = panel.sheet.cpu().numpy()
    assert np.array_equal(got, want)
    flat = got[0].transpose(2, 0, 1).reshape(-1)
    assert np.array_equal(flat[:256], np.arange(256)) and list(flat[768:773]) == [0, 255, 255, 0, 0]
    b = np.resize(probe, 3 * 4 * 10).reshape(3, 4, 10).astype(np.float32)      # 10 wide: the per-pixel path
    panel, want = single(lc.COLOR, b)
    assert np.array_equal(panel.sheet.cpu().numpy(), want)
    assert (want[0, :, 10:] == 0).all() and want.shape == (1, 4, 12, 3)
    m = np.resize(probe, 4 * 10).reshape(4, 10).astype(np.float32)             # a grey map, both paths
    for arr in (m, np.resize(probe[::-1], 8 * 40).reshape(8, 40).astype(np.float32)):
        panel, want = single(lc.MAP, arr)
        assert np.array_equal(panel.sheet.cpu().numpy(), want)


@pytest.mark.parametrize("name", list(lc.disp_cases()))
def test_disp_tiles_equal_the_recorded_normalize_image(name):
    z = np.load(os.path.join(GOLD, "logpanel.npz"))
    x = z["in_" + name]
    dtype = torch.bfloat16 if name.startswith("bf16") else torch.float32
    panel, want = single(lc.DISP, x, dtype)
    h, w = x.shape
    got = panel.sheet.cpu().numpy()
    stats = panel.stats.cpu().numpy()[0, 0]
    print(name, "stats", stats, "golden", z["stats_" + name], "bytes off", int((got[0, :, :w, 0] != z["bytes_" + name]).sum()))
    assert np.array_equal(stats.view(np.uint32), z["stats_" + name].view(np.uint32)) or \
        (np.isnan(stats).all() and np.isnan(z["stats_" + name]).all())
    assert np.array_equal(got[0, :, :w, 0], z["bytes_" + name])
    assert np.array_equal(got, want)                  # grey in three channels, zero padding


# ---------------------------------------------------------------------------------------------

def build_step(case: Case):
    """A golden case as the tensors a log step holds: inputs, outputs, T, and the fp32 warps
    of md2_generate_images."""
    cfg = case_config(case)
    colors, K, inv_K, noise = case_operands(case, DEV)
    frames = case.frame_ids
    disps = [case.disps[s].to(DEV) for s in range(4)]
    axis, trans = case.axisangle.to(DEV), case.translation.to(DEV)
    with torch.no_grad():
        if case.posecnn:
            from monodepth2_amd.trainer import posecnn_transforms
            st = case.inputs["stereo_T"].to(DEV) if "stereo_T" in case.inputs else None
            T = posecnn_transforms(disps, axis[:, :, 0], trans[:, :, 0], frames[1:], st, case.H, case.W,
                                   cfg.min_depth, cfg.max_depth, cfg.v1_multiscale)
        else:
            Ts, ti = [], 0
            for f in frames[1:]:
                if f == "s":
                    Ts.append(case.inputs["stereo_T"].to(DEV))
                else:
                    Ts.append(transformation_from_parameters(axis[ti], trans[ti], invert=(f < 0)))
                    ti += 1
            T = torch.stack(Ts, 0)
        outputs = {("disp", s): disps[s] for s in range(4)}
        up = None
        if cfg.predictive_mask:
            masks = {s: m.to(DEV) for s, m in case.masks.items()}
            outputs["predictive_mask"] = {("disp", s): masks[s] for s in range(4)}
            up, _ = predictive_mask_inputs(cfg, masks)
        _, sel = photometric_loss(cfg, disps, colors, K, inv_K, T, noise=noise, mask=up)
        if not cfg.disable_automasking:
            for s, m in selection_maps(cfg, sel.gt(cfg.noise_channels() - 1).float()).items():
                outputs["identity_selection/{}".format(s)] = m
        gen = generate_images(cfg, disps, colors, K, inv_K, T, want_depth=False, want_sample=False)["color"]
        inputs = {("K", 0): K[0], ("inv_K", 0): inv_K[0]}
        for s in range(4):
            for fi, f in enumerate(frames):
                c = colors[s][fi]
                if c is None:   # the fixtures keep the sources at scale 0 only: any picture will do
                    c = F.avg_pool2d(colors[0][fi], 2 ** s)
                inputs[("color", f, s)] = c
    return cfg, frames, inputs, outputs, T, gen


def expected_sheet(cfg, frames, inputs, outputs, gen, n):
    layout = panel_layout(cfg, frames, n, cfg.predictive_mask, not cfg.disable_automasking)
    return lc.expected_sheet(layout, frames, inputs, outputs, gen, n), layout


SMALL = ["mono_b2_64x128", "stereo_b2_64x128", "stereo_only_b2_64x128", "posecnn_b2_64x128",
         "v1_multiscale_b2_64x128", "predictive_mask_b2_32x64", "mono_bigpose_b2_64x96"]


@pytest.mark.parametrize("name", SMALL)
def test_panel_is_bitwise_the_quantised_generate_images_and_inputs(name):
    cfg, frames, inputs, outputs, T, gen = build_step(Case(name))
    panel = log_panel(cfg, inputs, outputs, frames, T)
    torch.cuda.synchronize()
    want, layout = expected_sheet(cfg, frames, inputs, outputs, gen, 2)
    got = panel.sheet.cpu().numpy()
    assert panel.layout == layout and got.shape == want.shape
    imgs = panel.images()
    for tag, (y, x, h, w) in layout[2].items():
        j = int(tag.rsplit("/", 1)[1])
        assert np.array_equal(imgs[tag].cpu().numpy(), want[j, y:y + h, x:x + w]), tag
    assert np.array_equal(got, want)
    st = panel.stats.cpu().numpy()
    for j in range(2):
        for s in range(4):
            d = outputs[("disp", s)][j].float().cpu().numpy()
            assert st[j, s, 0] == d.min() and st[j, s, 1] == d.max()
    assert any(t.startswith("color_pred_") for t in layout[2])
    assert sum(t.startswith("color_pred_") for t in layout[2]) == 2 * cfg.num_src


@pytest.mark.parametrize("name", ["full_mono_b2_192x640", "full_stereo_b2_192x640"])
def test_warps_against_the_references_own(name):
    cfg, frames, inputs, outputs, T, gen = build_step(Case(name))
    panel = log_panel(cfg, inputs, outputs, frames, T)
    imgs = {k: v.cpu().numpy() for k, v in panel.images().items() if k.startswith("color_pred_")}
    for f in frames[1:]:
        z = np.load(os.path.join(GOLD, "warp_{}_{}.npz".format(name, f)))
        want = z["q"]                                                    # (B, 3, H, W) bytes
        near = np.unpackbits(z["near"])[:want.size].reshape(want.shape).astype(bool)
        got = np.stack([imgs["color_pred_{}_0/{}".format(f, j)].transpose(2, 0, 1) for j in range(2)])
        diff = got.astype(np.int32) - want.astype(np.int32)
        print(name, f, "bytes off the reference's:", int((diff != 0).sum()), "of", diff.size, "largest step",
              int(np.abs(diff).max()), "near a step:", int(near.sum()))
        assert np.abs(diff).max() <= 1
        assert not (diff != 0)[~near].any()
    # and the same panel is bitwise the quantised md2_generate_images
    want, _ = expected_sheet(cfg, frames, inputs, outputs, gen, 2)
    assert np.array_equal(panel.sheet.cpu().numpy(), want)


@pytest.mark.parametrize("B", [5, 3, 1])
def test_only_the_first_four_items_and_every_byte_written(B):
    cfg = HotPathConfig(batch=B, height=32, width=80, num_src=2)
    frames = [0, -1, 1]
    inputs = synthetic_batch(B, 32, 80, frames, 4, seed=3, device=DEV)
    hp = synthetic_hotpath(B, 32, 80, num_src=2, seed=3, device=DEV)
    with torch.no_grad():
        T = torch.stack([transformation_from_parameters(hp["axisangle"][i], hp["translation"][i], invert=(f < 0))
                         for i, f in enumerate(frames[1:])])
        disps = [hp["disps"][s] for s in range(4)]
        colors = [[inputs[("color", f, s)] for f in frames] for s in range(4)]
        K, inv_K = [inputs[("K", s)] for s in range(4)], [inputs[("inv_K", s)] for s in range(4)]
        _, sel = photometric_loss(cfg, disps, colors, K, inv_K, T, seed=5)
        outputs = {("disp", s): disps[s] for s in range(4)}
        for s, m in selection_maps(cfg, sel.gt(cfg.num_src - 1).float()).items():
            outputs["identity_selection/%d" % s] = m
        gen = generate_images(cfg, disps, colors, K, inv_K, T, want_depth=False, want_sample=False)["color"]
    n = min(4, B)
    panel = log_panel(cfg, inputs, outputs, frames, T)
    assert panel.sheet.shape[0] == n and panel.stats.shape == (n, 4, 2)
    assert {int(t.rsplit("/", 1)[1]) for t in panel.layout[2]} == set(range(n))
    first = panel.sheet.clone()
    panel.sheet.fill_(0xAA)
    again = log_panel(cfg, inputs, outputs, frames, T, plan=panel.plan)
    assert again.plan is panel.plan and again.sheet.data_ptr() == panel.sheet.data_ptr()
    got = again.sheet.cpu().numpy()
    want, layout = expected_sheet(cfg, frames, inputs, outputs, gen, n)
    assert layout[2]["disp_3/0"][2:] == (4, 10)           # a width that is no multiple of 4
    assert np.array_equal(got, want) and np.array_equal(first.cpu().numpy(), want)
    cover = np.zeros(want.shape[1:3], bool)
    for tag, (y, x, h, w) in layout[2].items():
        cover[y:y + h, x:x + w] = True
    assert (~cover).any() and (got[:, ~cover] == 0).all()


def test_capture_replays_equal_eager_without_allocating():
    cfg, frames, inputs, outputs, T, _ = build_step(Case("mono_b2_64x128"))
    a = log_panel(cfg, inputs, outputs, frames, T)
    ref0 = a.sheet.clone()
    b = log_panel(cfg, inputs, outputs, frames, T)             # a second eager run, its own buffers
    assert b.sheet.data_ptr() != a.sheet.data_ptr() and torch.equal(b.sheet, ref0)
    plan = a.plan
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        log_panel(cfg, inputs, outputs, frames, T, plan=plan)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for it in range(2):
        with torch.no_grad():                                  # new values in the same storages
            for s in range(4):
                outputs[("disp", s)].copy_(torch.rand(outputs[("disp", s)].shape, device=DEV, generator=gen))
            for f in (0, -1):
                inputs[("color", f, 0)].copy_(torch.rand(inputs[("color", f, 0)].shape, device=DEV, generator=gen))
            T.add_(0.001 * (it + 1))
        eager = log_panel(cfg, inputs, outputs, frames, T).sheet.clone()
        plan.sheet.fill_(0x55)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        graph.replay()
        after = torch.cuda.memory_stats()["allocation.all.allocated"]
        torch.cuda.synchronize()
        assert after == before
        assert torch.equal(plan.sheet, eager) and not torch.equal(eager, ref0)
