"""GPU tests of the disparity-picture operator (csrc/viz.hip, viz_ops.colorize_disparity)
and of single-image inference (monodepth2_amd.infer).

Yardsticks: tests/viz_case.py, the numpy restatement of md2_disp_colorize in the kernel's
written order — compared bitwise (the resized map and the statistics as uint32 views) and
bytewise — and tests/golden/viz/viz.npz, captured from numpy, matplotlib and torch for
test_simple.py:136-155.  At the identity size the kernel must give the libraries' bytes
exactly.  The resize is held to measured bars: torch's CPU kernel rounds the same formula in
another order, so the kernel's distance from the recorded fp64 evaluation may be 4 x the
floor torch leaves (a wrong weight misses by orders of magnitude), and against the
libraries' bytes a pixel may differ only by one table step, in at most 0.5 % of an image.
Bitwise parity rests on nothing being contracted into an fma and on the device's fp32 and
fp64 division being correctly rounded under the default compiler flags.
"""
import functools

import numpy as np
import pytest
import torch

import viz_case as vc
from monodepth2_amd.viz_ops import colorize_disparity, workspace_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"
EXACT = [n for n in vc.build_cases() if n.startswith("e_")]
RESIZE = [n for n in vc.build_cases() if n.startswith("r_")]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def golden():
    return vc.load_golden()


@functools.lru_cache(maxsize=None)
def lut():
    return vc.load_lut(golden())


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's (rgb, resized, stats) of a golden case: computed once, shared."""
    c = vc.case(golden(), name)
    out = vc.colorize_np(c["disp"], c["size"], c["percentile"], lut())
    for a in out:
        a.setflags(write=False)
    return out


def run(name):
    c = vc.case(golden(), name)
    rgb, resized, stats = colorize_disparity(cuda(c["disp"]), c["size"], c["percentile"], return_resized=True,
                                             return_stats=True)
    B = c["disp"].shape[0]
    assert rgb.shape == (B,) + c["size"] + (3,) and rgb.dtype == torch.uint8 and rgb.is_cuda
    assert resized.shape == (B,) + c["size"] and resized.dtype == torch.float32
    assert stats.shape == (B, 2) and stats.dtype == torch.float32
    return c, rgb.cpu().numpy(), resized.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("name", EXACT + RESIZE)
def test_kernel_is_bit_equal_to_the_restatement(name):
    _, rgb, resized, stats = run(name)
    want_rgb, want_resized, want_stats = expected(name)
    with np.errstate(all="ignore"):
        print(name, "stats", stats.tolist(), "restatement", want_stats.tolist(), "max |resized diff|",
              float(np.nanmax(np.abs(resized - want_resized))), "bytes off", int((rgb != want_rgb).sum()))
    if name == "e_nan_16x32":       # NaN payloads are not part of the contract
        assert np.array_equal(np.isnan(resized), np.isnan(want_resized)) and np.isnan(stats).all()
        keep = ~np.isnan(want_resized)
        assert np.array_equal(bits(resized[keep]), bits(want_resized[keep]))
    else:
        assert np.array_equal(bits(resized), bits(want_resized))
        assert np.array_equal(bits(stats), bits(want_stats))
    assert np.array_equal(rgb, want_rgb)


@pytest.mark.parametrize("name", EXACT)
def test_kernel_is_byte_equal_to_the_golden_at_the_identity_size(name):
    c, rgb, _, stats = run(name)
    print(name, "bytes off the golden", int((rgb != c["rgb"]).sum()), "of", rgb.size)
    assert np.array_equal(rgb, c["rgb"])
    if name != "e_nan_16x32":
        assert np.array_equal(bits(stats[:, 0]), bits(c["vmin"])) and np.array_equal(bits(stats[:, 1]), bits(c["vmax"]))


@pytest.mark.parametrize("name", RESIZE)
def test_resize_is_within_four_floors_of_fp64(name):
    c, _, resized, _ = run(name)
    err = float(np.abs(resized.astype(np.float64) - c["f64"]).max())
    print(name, "max |kernel - fp64|", err, "floor (torch CPU)", c["floor"], "=", err / c["floor"], "floors")
    assert err <= 4 * c["floor"]


@pytest.mark.parametrize("name", RESIZE)
def test_resize_cases_against_the_reference_bytes(name):
    c, rgb, _, _ = run(name)
    a, b = vc.lut_index(c["rgb"], lut()), vc.lut_index(rgb, lut())
    off = a != b
    print(name, "pixels off the golden", int(off.sum()), "of", off.size, "largest table step",
          int(np.abs(a - b).max()))
    assert np.abs(a - b).max() <= 1          # only where the index is one step away
    assert off.mean() <= 0.005               # and at most 0.5 % of the image


def test_batch_of_three_equals_three_single_calls():
    c = vc.case(golden(), "e_batch3_16x32")
    disp = cuda(c["disp"])
    for size in (None, (37, 50)):
        whole = colorize_disparity(disp, size, return_resized=True, return_stats=True)
        singles = [colorize_disparity(disp[i:i + 1], size, return_resized=True, return_stats=True) for i in range(3)]
        for j in range(3):
            assert torch.equal(whole[j], torch.cat([s[j] for s in singles]))
        assert not torch.equal(whole[2][0], whole[2][1])      # statistics per image, not pooled


def test_bitwise_repeatable_and_capturable():
    c = vc.case(golden(), "r_24x80_47x155")
    disp = cuda(np.concatenate([c["disp"], c["disp"][:, :, ::-1, :] * np.float32(0.5)]))
    a = colorize_disparity(disp, c["size"], return_resized=True, return_stats=True)
    b = colorize_disparity(disp, c["size"], return_resized=True, return_stats=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert np.array_equal(a[0][0].cpu().numpy(), expected("r_24x80_47x155")[0][0])
    ws = torch.empty(workspace_bytes(2, (24, 80), c["size"]), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        colorize_disparity(disp, c["size"], return_resized=True, return_stats=True, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = colorize_disparity(disp, c["size"], return_resized=True, return_stats=True, workspace=ws)
    replays = []
    for _ in range(2):
        out[0].fill_(7), out[1].fill_(-1.0), out[2].fill_(-1.0)
        graph.replay()
        replays.append([o.clone() for o in out])
    torch.cuda.synchronize()
    for r in replays:
        for x, y in zip(r, a):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_nan_image_is_black_and_its_neighbours_are_untouched():
    g = golden()
    holed, ok = vc.case(g, "e_nan_16x32"), vc.case(g, "e_16x32")
    disp = cuda(np.concatenate([ok["disp"], holed["disp"], ok["disp"] * np.float32(0.5)]))
    rgb, stats = colorize_disparity(disp, return_stats=True)
    rgb, stats = rgb.cpu().numpy(), stats.cpu().numpy()
    assert not rgb[1].any() and np.isnan(stats[1]).all()
    assert np.array_equal(rgb[0], ok["rgb"][0]) and np.array_equal(rgb[0], expected("e_16x32")[0][0])
    want = vc.colorize_np(ok["disp"] * np.float32(0.5), None, 95, lut())
    assert np.array_equal(rgb[2], want[0][0]) and np.array_equal(bits(stats[2]), bits(want[2][0]))
    assert rgb[0].any() and rgb[2].any()


def test_caller_workspace_with_garbage_and_input_checks():
    c = vc.case(golden(), "e_47x155")
    need = workspace_bytes(1, (47, 155), (47, 155))
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    rgb = colorize_disparity(cuda(c["disp"]), workspace=ws)
    assert np.array_equal(rgb.cpu().numpy(), c["rgb"])
    rgb = colorize_disparity(cuda(c["disp"][:, 0]))                       # (B, h, w) as well
    assert np.array_equal(rgb.cpu().numpy(), c["rgb"])
    with pytest.raises(ValueError, match="workspace"):
        colorize_disparity(cuda(c["disp"]), workspace=ws[:need - 256])
    with pytest.raises(ValueError, match="float32"):
        colorize_disparity(cuda(c["disp"]).double())
    with pytest.raises(ValueError, match="percentile"):
        colorize_disparity(cuda(c["disp"]), percentile=94.5)
    with pytest.raises(RuntimeError, match="percentile"):
        colorize_disparity(cuda(c["disp"]), percentile=101)


# ---- inference ---------------------------------------------------------------------------

# The smallest feed size of this aspect the networks accept: the encoder halves five times and
# the decoder's ReflectionPad2d(1) is undefined on a map one pixel high, so 32 x 64 (a 1 x 2
# deepest map) is refused by stock PyTorch as well ("Padding size should be less than the
# corresponding input dimension"); 64 x 128 gives 2 x 4.
FEED = (64, 128)
ORIGINAL = (37, 50)


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """A random-weight ResNet-18 checkpoint with feed size 64 x 128 and two lossless 37 x 50
    PNGs in one folder."""
    from PIL import Image
    from monodepth2_amd import networks
    root = tmp_path_factory.mktemp("infer")
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False)
    dec = networks.DepthDecoder(enc.num_ch_enc)
    state = enc.state_dict()
    state["height"], state["width"], state["use_stereo"] = FEED[0], FEED[1], False
    (root / "weights").mkdir()
    torch.save(state, root / "weights" / "encoder.pth")
    torch.save(dec.state_dict(), root / "weights" / "depth.pth")
    (root / "images").mkdir()
    rng = np.random.RandomState(3)
    yy, xx = np.meshgrid(np.arange(ORIGINAL[0]), np.arange(ORIGINAL[1]), indexing="ij")
    for i, name in enumerate(("a", "b")):
        img = np.stack([(yy * 5 + xx * 3 + 40 * i) % 256, (xx * 4 + 17) % 256, (yy * 6 + 90 * i) % 256], 2)
        img = np.clip(img + rng.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(root / "images" / (name + ".png"))
    return root


def test_preprocess_equals_pil_lanczos(demo):
    from PIL import Image
    from monodepth2_amd.infer import preprocess
    for name in ("a", "b"):
        img = Image.open(demo / "images" / (name + ".png")).convert("RGB")
        got = preprocess(img, FEED, DEV)
        assert got.shape == (1, 3) + FEED and got.dtype == torch.float32 and got.is_cuda
        want = np.array(img.resize((FEED[1], FEED[0]), Image.LANCZOS), dtype=np.uint8)
        want = torch.from_numpy(want).permute(2, 0, 1).unsqueeze(0).float().div(255)
        assert np.array_equal(bits(got), bits(want))
        again = preprocess(np.asarray(img), FEED, DEV)          # an array, through the cached plan
        assert torch.equal(again, got)


def test_infer_main_writes_the_reference_files(demo, capsys, monkeypatch):
    """`infer.main` on a folder, on one file with --pred_metric_depth, and on a folder that
    holds only a *_disp.jpg.  The saved arrays and the pictures are compared, bitwise and
    bytewise, with disp_to_depth and the restatement applied to what predict_disparities
    returned for the very tensor `preprocess` made — the forward pass that produced the
    files, recorded by a wrapper.  A second forward pass is not the yardstick: the networks'
    eval-mode convolutions (MIOpen's, at this size) are not bitwise repeatable from call to
    call — 500-600 of 16 384 disparities move by one fp32 ulp (6e-8) between any two calls
    on one tensor, measured on an MI355X — so an independent pass is held to 1e-5, the bar
    tests/test_pose_eval_gpu.py uses for the same networks' fp32 rounding of values below 1."""
    from PIL import Image
    from monodepth2_amd import infer
    from monodepth2_amd.evaluate_depth import STEREO_SCALE_FACTOR, predict_disparities
    from monodepth2_amd.layers import disp_to_depth
    images = demo / "images"
    weights = str(demo / "weights")
    calls = []

    def recording(encoder, decoder, x, *args, **kwargs):
        disp = predict_disparities(encoder, decoder, x, *args, **kwargs)
        calls.append((x.clone(), disp.clone()))
        return disp

    monkeypatch.setattr(infer, "predict_disparities", recording)
    infer.main(["--image_path", str(images), "--load_weights_folder", weights, "--ext", "png"])
    text = capsys.readouterr().out
    assert "-> Predicting on 2 test images" in text and "-> Done!" in text
    assert "   Processed 2 of 2 images - saved predictions to:" in text
    assert sorted(p.name for p in images.iterdir()) == ["a.png", "a_disp.jpeg", "a_disp.npy", "b.png", "b_disp.jpeg",
                                                         "b_disp.npy"]

    enc, dec, feed = infer.load_networks(weights, 18, DEV)
    assert feed == FEED
    pil_images = [Image.open(images / (n + ".png")).convert("RGB") for n in ("a", "b")]
    x = torch.cat([infer.preprocess(im, feed, DEV) for im in pil_images])
    assert len(calls) == 1 and torch.equal(calls[0][0], x)          # one pass, on the preprocessed images
    disp = calls[0][1]
    assert disp.shape == (2, 1) + FEED and disp.dtype == torch.float32
    scaled, _ = disp_to_depth(disp, 0.1, 100)
    independent = disp_to_depth(predict_disparities(enc, dec, x), 0.1, 100)[0]
    print("saved vs an independent forward pass: max abs diff", float((independent - scaled).abs().max()))
    for i, n in enumerate(("a", "b")):
        saved = np.load(images / (n + "_disp.npy"))
        assert saved.shape == (1, 1) + FEED and saved.dtype == np.float32
        assert np.array_equal(bits(saved), bits(scaled[i:i + 1]))
        assert np.allclose(saved, independent[i:i + 1].cpu().numpy(), rtol=0, atol=1e-5)
        with Image.open(images / (n + "_disp.jpeg")) as jpeg:      # lossy: existence and shape only
            assert jpeg.size == (ORIGINAL[1], ORIGINAL[0]) and jpeg.mode == "RGB"

    results = infer.predict_images(enc, dec, pil_images, feed)
    assert len(calls) == 2 and torch.equal(calls[1][0], x)
    disp = calls[1][1]
    scaled, _ = disp_to_depth(disp, 0.1, 100)
    want_rgb, _, _ = vc.colorize_np(disp.cpu().numpy(), ORIGINAL, 95, lut())
    for i in range(2):
        assert results[i][0].shape == (1, 1) + FEED and results[i][0].dtype == np.float32
        assert np.array_equal(bits(results[i][0]), bits(scaled[i:i + 1]))
        assert results[i][1].shape == ORIGINAL + (3,) and results[i][1].dtype == np.uint8
        assert np.array_equal(results[i][1], want_rgb[i])
    assert not np.array_equal(want_rgb[0], want_rgb[1])

    # one file, metric depth: NAME_depth.npy; a *_disp.jpg input is skipped
    (images / "old_disp.jpg").write_bytes(b"not an image")
    infer.main(["--image_path", str(images / "a.png"), "--load_weights_folder", weights, "--pred_metric_depth"])
    metric = np.load(images / "a_depth.npy")
    assert len(calls) == 3 and torch.equal(calls[2][0], x[:1])
    assert np.array_equal(bits(metric), bits(STEREO_SCALE_FACTOR * disp_to_depth(calls[2][1], 0.1, 100)[1]))
    assert "   Processed 1 of 1 images - saved predictions to:" in capsys.readouterr().out
    infer.main(["--image_path", str(images), "--load_weights_folder", weights])      # --ext jpg: only old_disp.jpg
    text = capsys.readouterr().out
    assert "-> Predicting on 1 test images" in text and "Processed" not in text and "-> Done!" in text
    assert len(calls) == 3
