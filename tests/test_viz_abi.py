"""CPU-side checks of the disparity-picture ABI (md2_disp_colorize, csrc/viz.hip): struct
layout, every refusal and its message, workspace sizes — no kernel is launched — the magma
table (golden, the kernel's source, the installed matplotlib), and the pin of the tests'
numpy restatement (tests/viz_case.py) to the golden captured from numpy, matplotlib and
torch (tests/golden/viz/make_viz_golden.py, for test_simple.py:136-155)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib
from monodepth2_amd.build import CSRC, build
from monodepth2_amd.viz_ops import colorize_disparity, viz_desc, workspace_bytes

import viz_case as vc


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return vc.load_golden()


def test_struct_layout_and_abi(L):
    D = _lib.VizDesc
    assert ctypes.sizeof(D) == 32
    assert (D.batch.offset, D.in_height.offset, D.in_width.offset, D.out_height.offset) == (0, 4, 8, 12)
    assert (D.out_width.offset, D.percentile.offset, D.flags.offset, D.reserved.offset) == (16, 20, 24, 28)
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert {"md2_disp_colorize", "md2_disp_colorize_workspace_bytes"} <= set(_lib.EXPORTS)
    assert hasattr(L, "md2_disp_colorize") and hasattr(L, "md2_disp_colorize_workspace_bytes")


def desc(**kw):
    args = dict(batch=2, in_hw=(16, 32), out_hw=(37, 50), percentile=95)
    for k in ("in_height", "in_width", "out_height", "out_width"):
        if k in kw:
            side = "in_hw" if k.startswith("in") else "out_hw"
            hw = list(args[side])
            hw[0 if k.endswith("height") else 1] = kw.pop(k)
            args[side] = tuple(hw)
    args.update(kw)
    return viz_desc(**args)


BAD = [
    (dict(batch=0), "must be positive"),
    (dict(batch=-1), "must be positive"),
    (dict(in_height=0), "must be positive"),
    (dict(in_width=-5), "must be positive"),
    (dict(out_height=0), "must be positive"),
    (dict(out_width=0), "must be positive"),
    (dict(batch=65536), "65535"),                       # images are grid.y
    (dict(out_hw=(4096, 4097)), "2^24"),                # f32(n - 1) must be exact
    (dict(out_hw=(2 ** 16, 2 ** 16)), "2^24"),          # also past int32
    (dict(in_hw=(2 ** 16, 2 ** 15)), "2^31"),
    (dict(percentile=-1), "percentile"),
    (dict(percentile=101), "percentile"),
]


def call(L, d, ptrs):
    return L.md2_disp_colorize(ctypes.byref(d) if d is not None else None, *ptrs, None)


@pytest.mark.parametrize("kw,msg", BAD)
def test_invalid_desc_is_refused_with_a_message(L, kw, msg):
    d = desc(**kw)
    dummy = ctypes.c_void_p(256)   # non-NULL, never dereferenced: the desc is refused first
    assert L.md2_disp_colorize_workspace_bytes(ctypes.byref(d)) == 0
    assert msg in L.md2_last_error().decode()
    assert call(L, d, [dummy] * 5) == -1
    assert msg in L.md2_last_error().decode()
    with pytest.raises(RuntimeError, match="md2_disp_colorize_workspace_bytes"):
        workspace_bytes(d.batch, (d.in_height, d.in_width), (d.out_height, d.out_width), d.percentile)


def test_the_largest_legal_sizes_are_accepted(L):
    d = desc(batch=65535, out_hw=(4096, 4096), percentile=100)
    assert L.md2_disp_colorize_workspace_bytes(ctypes.byref(d)) >= 4 * 65535 * 2 ** 24
    for p in (0, 100):
        assert L.md2_disp_colorize_workspace_bytes(ctypes.byref(desc(batch=1, in_hw=(1, 1), out_hw=(1, 1),
                                                                       percentile=p))) > 0


def test_null_desc_and_operands(L):
    assert L.md2_disp_colorize_workspace_bytes(None) == 0
    assert "NULL desc" in L.md2_last_error().decode()
    x = ctypes.c_void_p(256)
    assert call(L, None, [x] * 5) == -1
    assert "NULL desc" in L.md2_last_error().decode()
    d = desc()
    for hole in (0, 1, 4):          # disp, rgb, workspace; resized (2) and stats (3) are optional
        args = [x] * 5
        args[hole] = None
        assert call(L, d, args) == -1
        assert "NULL operand" in L.md2_last_error().decode()


def test_flags_and_misaligned_workspace(L):
    d = desc()
    d.flags = 1
    assert L.md2_disp_colorize_workspace_bytes(ctypes.byref(d)) == 0
    assert "flags" in L.md2_last_error().decode()
    assert call(L, d, [ctypes.c_void_p(256)] * 5) == -1
    assert "flags" in L.md2_last_error().decode()
    d, x = desc(), ctypes.c_void_p(256)
    for off in (8, 16, 128):
        assert call(L, d, [x] * 4 + [ctypes.c_void_p(256 + off)]) == -1
        assert "256-byte aligned" in L.md2_last_error().decode()


def test_workspace_is_monotone_in_batch_and_size(L):
    def ws(batch, out_hw):
        n = L.md2_disp_colorize_workspace_bytes(ctypes.byref(desc(batch=batch, out_hw=out_hw)))
        assert n % 256 == 0 and n >= 4 * batch * out_hw[0] * out_hw[1]   # the resized maps stay in it
        return n

    by_batch = [ws(b, (37, 50)) for b in (1, 2, 3, 16, 697, 65535)]
    assert all(a < b for a, b in zip(by_batch, by_batch[1:])), by_batch
    by_size = [ws(3, s) for s in ((1, 1), (3, 5), (37, 50), (47, 155), (375, 1242), (1024, 1025), (4096, 4096))]
    assert all(a <= b for a, b in zip(by_size, by_size[1:])), by_size
    assert by_size[0] < by_size[2] < by_size[-1]
    # neither the input size nor the percentile enters
    a = L.md2_disp_colorize_workspace_bytes(ctypes.byref(desc(in_hw=(1, 1), percentile=0)))
    assert a == L.md2_disp_colorize_workspace_bytes(ctypes.byref(desc(in_hw=(192, 640), percentile=100)))
    assert workspace_bytes(2, (16, 32), (37, 50)) == a


def test_colorize_disparity_has_no_cpu_fallback_and_checks_its_input():
    with pytest.raises(RuntimeError, match="GPU only"):
        colorize_disparity(torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        colorize_disparity(np.zeros((1, 1, 4, 4), np.float32))


def test_inference_refuses_a_feed_size_the_networks_cannot_take(tmp_path):
    from monodepth2_amd import infer
    image = np.zeros((37, 50, 3), np.uint8)
    for feed in ((32, 64), (64, 100), (96, 32)):
        with pytest.raises(ValueError, match="multiple of 32 and at least 64 x 64"):
            infer.predict_images(None, None, [image], feed)
    assert infer.predict_images(None, None, [], (64, 128)) == []
    torch.save({"conv1.weight": torch.zeros(1)}, tmp_path / "encoder.pth")
    with pytest.raises(SystemExit, match="height / width"):
        infer.load_networks(str(tmp_path), 18, "cpu")
    args = infer.parse_args(["--image_path", "x", "--load_weights_folder", "w"])
    assert (args.ext, args.num_layers, args.pred_metric_depth) == ("jpg", 18, False)
    with pytest.raises(SystemExit):
        infer.parse_args(["--image_path", "x", "--load_weights_folder", "w", "--model_name", "mono_640x192"])


def test_the_magma_table_is_pinned(golden):
    lut = vc.load_lut(golden)
    assert len({tuple(r) for r in lut}) == 256
    # the kernel's constant array, read from its source: R | G << 8 | B << 16
    src = open(os.path.join(CSRC, "viz.hip")).read()
    body = re.search(r"kMagma\[256\] = \{(.*?)\};", src, re.S).group(1)
    words = np.array([int(w, 16) for w in re.findall(r"0x[0-9a-fA-F]+", body)], np.uint32)
    assert words.shape == (256,)
    mine = np.stack([words & 255, (words >> 8) & 255, (words >> 16) & 255], 1).astype(np.uint8)
    assert np.array_equal(mine, lut)
    matplotlib = pytest.importorskip("matplotlib")
    live = (matplotlib.colormaps["magma"](np.arange(256))[:, :3] * 255).astype(np.uint8)
    assert np.array_equal(live, lut)


def test_golden_is_complete(golden):
    exact, resize = vc.case_names(golden, "e"), vc.case_names(golden, "r")
    assert len(exact) == 13 and len(resize) == 4
    assert sorted(exact + resize) == sorted(vc.build_cases())
    for name, (disp, size, pct) in vc.build_cases().items():     # the inputs are regenerated identically
        c = vc.case(golden, name)
        assert np.array_equal(c["disp"].view(np.uint32), disp.view(np.uint32)) and c["size"] == size
        assert c["percentile"] == pct and c["rgb"].shape == (disp.shape[0],) + size + (3,)
    for name in resize:
        c = vc.case(golden, name)
        assert 0 < c["floor"] < 1e-6 and c["f64"].dtype == np.float64
    assert {vc.case(golden, n)["percentile"] for n in exact} == {0, 50, 95, 100}
    assert vc.case(golden, "e_batch3_16x32")["disp"].shape[0] == 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", [n for n in vc.build_cases() if n.startswith("e_")])
def test_restatement_reproduces_the_exact_stage_golden(golden, name):
    """At the identity size the resize returns the input, and everything after it — numpy's
    percentile, the minimum, matplotlib's Normalize and colormap, the uint8 conversion — is
    restated exactly: vmin and vmax bit-equal, every byte equal, none excluded."""
    c = vc.case(golden, name)
    rgb, resized, stats = vc.colorize_np(c["disp"], c["size"], c["percentile"], vc.load_lut(golden))
    if name == "e_nan_16x32":
        # the written formula spreads the NaN to the neighbours whose zero weight multiplies
        # it (torch's kernel skips them); the image is all "bad" either way
        keep = ~np.isnan(resized)
        assert np.isnan(c["resized"]).sum() == 1 and 1 <= (~keep).sum() <= 4
        assert np.array_equal(resized[keep], c["resized"][keep])
        assert np.isnan(stats).all() and np.isnan(c["vmin"]).all() and np.isnan(c["vmax"]).all()
        assert not c["rgb"].any()
    else:
        assert np.array_equal(bits(resized), bits(c["resized"]))
        assert np.array_equal(bits(stats[:, 0]), bits(c["vmin"])), (stats[:, 0], c["vmin"])
        assert np.array_equal(bits(stats[:, 1]), bits(c["vmax"])), (stats[:, 1], c["vmax"])
    assert np.array_equal(rgb, c["rgb"])


@pytest.mark.parametrize("name", [n for n in vc.build_cases() if n.startswith("r_")])
def test_restatement_of_the_resize_is_within_the_golden_bars(golden, name):
    """The fp32 resize in the kernel's order against the recorded fp64 evaluation (4 x the
    floor torch's CPU kernel leaves) and against the libraries' bytes (a differing pixel one
    table step away, at most 0.5 % of them): the bars of the GPU tests, on the host."""
    c = vc.case(golden, name)
    lut = vc.load_lut(golden)
    rgb, resized, _ = vc.colorize_np(c["disp"], c["size"], c["percentile"], lut)
    err = float(np.abs(resized.astype(np.float64) - c["f64"]).max())
    a, b = vc.lut_index(c["rgb"], lut), vc.lut_index(rgb, lut)
    print(name, "max |restatement - fp64|", err, "floor", c["floor"], "pixels off", int((a != b).sum()), "of", a.size)
    assert err <= 4 * c["floor"]
    assert np.abs(a - b).max() <= 1 and (a != b).mean() <= 0.005
