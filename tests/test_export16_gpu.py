"""eval_ops.benchmark_depth_maps (md2_depth_export16, csrc/eval.hip) against the fp64 numpy
restatement of the reference's benchmark export (tests/export16_case.py).

The rule: equality is exact except where the fp64 value depth * 256 lies within 1e-6 of an
integer (truncation is discontinuous there), where one count is allowed; such pixels are at
most 0.01 % of the unclipped ones; every pixel whose fp64 depth is at least 80 * (1 + 1e-9)
is exactly 20480.  Sizes: the benchmark's own, odd widths and odd per-image offsets (where
the 8- and 4-byte stores must give way to 2-byte ends), a downscale, the identity, and the
one-pixel ends."""
import numpy as np
import pytest
import torch

import export16_case as xc

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (input, output, B)
SIZES = [((24, 80), (352, 1216), 3),   # the straddling inputs
         ((24, 80), (37, 125), 3),     # odd width; odd per-image offsets
         ((40, 96), (17, 33), 2),      # downscale
         ((16, 32), (16, 32), 1),      # identity
         ((1, 1), (3, 5), 1),
         ((5, 7), (1, 1), 2)]


def inputs(in_hw, B):
    if in_hw == (24, 80) and B == 3:
        return xc.straddling_inputs()
    return xc.smooth_inputs(B, in_hw[0], in_hw[1], seed=11)


@pytest.fixture(scope="module")
def cases():
    """(sig, sigf) per size, made once."""
    return {(i, o, B): inputs(i, B) for i, o, B in SIZES}


def run(sig, sigf, out_hw, **kw):
    from monodepth2_amd.eval_ops import benchmark_depth_maps
    d = torch.from_numpy(sig).to(DEV)
    f = torch.from_numpy(sigf).to(DEV) if sigf is not None else None
    out = benchmark_depth_maps(d, f, out_hw=out_hw, **kw)
    assert out.dtype == torch.int16 and tuple(out.shape) == (sig.shape[0],) + tuple(out_hw) and out.is_cuda
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("pp", [True, False])
@pytest.mark.parametrize("in_hw,out_hw,B", SIZES)
def test_matches_the_fp64_restatement(cases, in_hw, out_hw, B, pp):
    sig, sigf = cases[(in_hw, out_hw, B)]
    flipped = sigf if pp else None
    xc.compare(run(sig, flipped, out_hw), sig, flipped, out_hw)


@pytest.mark.parametrize("in_hw,out_hw,B", SIZES)
def test_already_scaled_input(cases, in_hw, out_hw, B):
    """min_depth 1 with max_depth inf makes disp_to_depth the identity: what
    --ext_disp_to_eval files hold goes in as it is."""
    import eval_case as ec
    sig, _ = cases[(in_hw, out_hw, B)]
    scaled = ec.scaled_disp(sig)
    kw = dict(min_depth=1.0, max_depth=float("inf"))
    got = run(scaled, None, out_hw, **kw)
    xc.compare(got, scaled, None, out_hw, **kw)
    # and it is the same map the raw disparities give
    assert np.array_equal(got, run(sig, None, out_hw))


def test_other_constants(cases):
    sig, sigf = cases[((24, 80), (37, 125), 3)]
    kw = dict(scale_factor=1.0, clip_max=50.0, quant=1000.0, min_depth=0.5, max_depth=60.0)
    xc.compare(run(sig, sigf, (37, 125), **kw), sig, sigf, (37, 125), **kw)


def test_the_three_edge_values():
    sig = np.empty((4, 1, 3, 5), np.float32)
    for b, v in enumerate((0.0, -0.25, np.nan, 0.5)):
        sig[b] = v
    got = run(sig, None, (4, 7), min_depth=1.0, max_depth=float("inf"))
    assert (got[0] == 20480).all()            # 5.4 / 0 -> clip_max * quant
    assert (got[1] == 0).all()                # negative -> 0
    assert (got[2] == 0).all()                # NaN -> 0
    assert (got[3] == int(5.4 / 0.5 * 256)).all()
    assert np.array_equal(got, xc.export16_np(sig, None, (4, 7), np.float64, min_depth=1.0, max_depth=float("inf")))


def test_repeatable_and_stream_independent(cases):
    sig, sigf = cases[((24, 80), (352, 1216), 3)]
    from monodepth2_amd.eval_ops import benchmark_depth_maps
    d, f = torch.from_numpy(sig).to(DEV), torch.from_numpy(sigf).to(DEV)
    a = benchmark_depth_maps(d, f)
    b = benchmark_depth_maps(d, f)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = benchmark_depth_maps(d, f)
    side.synchronize()
    assert torch.equal(a, c)


@pytest.mark.parametrize("out_hw,B", [((37, 125), 3), ((5, 6), 2), ((3, 1), 3), ((352, 1216), 1)])
def test_out_view_at_an_odd_offset_leaves_its_surroundings_alone(cases, out_hw, B):
    """`out` a view one element into a larger sentinel-filled buffer: the maps are the same
    as in a buffer of their own, and no sentinel changes (a wide store running over an odd
    row end or image end would hit one)."""
    from monodepth2_amd.eval_ops import benchmark_depth_maps
    sig, sigf = cases[((24, 80), (352, 1216), 3)]
    d, f = torch.from_numpy(sig[:B]).to(DEV), torch.from_numpy(sigf[:B]).to(DEV)
    own = benchmark_depth_maps(d, f, out_hw=out_hw)
    n = B * out_hw[0] * out_hw[1]
    pad, sentinel = 16, 0x5A5A
    for offset in (1, 2, 3):
        buf = torch.full((n + 2 * pad,), sentinel, dtype=torch.int16, device=DEV)
        view = buf[offset:offset + n].view(B, *out_hw)
        assert view.data_ptr() == buf.data_ptr() + 2 * offset
        got = benchmark_depth_maps(d, f, out_hw=out_hw, out=view)
        assert got.data_ptr() == view.data_ptr()
        assert torch.equal(view, own), offset
        assert bool((buf[:offset] == sentinel).all()) and bool((buf[offset + n:] == sentinel).all()), offset
    with pytest.raises(ValueError, match="out must be"):
        benchmark_depth_maps(d, f, out_hw=out_hw, out=torch.empty((B,) + out_hw, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="out must be"):
        benchmark_depth_maps(d, f, out_hw=out_hw, out=torch.empty((B + 1,) + out_hw, dtype=torch.int16, device=DEV))


def test_input_checks():
    from monodepth2_amd.eval_ops import benchmark_depth_maps
    d = torch.rand(2, 1, 4, 8, device=DEV)
    with pytest.raises(ValueError, match="expected disp"):
        benchmark_depth_maps(d[0, 0])
    with pytest.raises(ValueError, match="float32"):
        benchmark_depth_maps(d.double())
    with pytest.raises(ValueError, match="post_process_disp must match"):
        benchmark_depth_maps(d, d[:1])
    with pytest.raises(RuntimeError, match="65535"):
        benchmark_depth_maps(d, quant=1024.0)
    with pytest.raises(RuntimeError, match="must be positive"):
        benchmark_depth_maps(d, out_hw=(0, 8))


def test_write_benchmark_pngs(cases, tmp_path):
    from PIL import Image

    from monodepth2_amd.eval_ops import benchmark_depth_maps, write_benchmark_pngs
    sig, sigf = cases[((24, 80), (352, 1216), 3)]
    maps = benchmark_depth_maps(torch.from_numpy(sig).to(DEV), torch.from_numpy(sigf).to(DEV))
    paths = write_benchmark_pngs(maps, str(tmp_path / "benchmark_predictions"))
    assert [p.name for p in sorted((tmp_path / "benchmark_predictions").iterdir())] == \
        ["0000000000.png", "0000000001.png", "0000000002.png"]
    want = maps.cpu().numpy().view(np.uint16)
    assert want.max() == 20480 and want.min() > 0   # image 1 reaches the clip
    for p, m in zip(paths, want):
        with Image.open(p) as im:
            assert im.mode == "I;16" and im.size == (1216, 352)
            assert np.array_equal(np.asarray(im), m)
