"""The stem's fused BatchNorm passes (md2_bn_pool_fwd, md2_bn_bwd_reduce_mask +
md2_stem_wgrad_bn, stem_ops.stem_bn_pool) against the separate launches of the same
build (md2_bn_fwd_mask + md2_maxpool3s2_fwd, md2_bn_bwd_mask + md2_stem_wgrad), which the
fp64 comparisons of test_bnorm_gpu.py / test_stem_gpu.py cover.  A folded pass must give
the bits of the pass it replaces: every comparison here is bitwise."""
import copy
import ctypes

import pytest
import torch

from monodepth2_amd import _lib, bn_ops, conv_ops, stem_ops
from monodepth2_amd.networks import ResnetEncoder

pytestmark = pytest.mark.gpu

CL = torch.channels_last
EPS, MOM = 1e-5, 0.1


@pytest.fixture(autouse=True)
def _enabled(monkeypatch):
    for name in ("ENABLED", "FWD_ENABLED", "FUSE", "FUSE_FWD", "FUSE_WGRAD"):
        monkeypatch.setattr(stem_ops, name, True)
    monkeypatch.setattr(bn_ops, "ENABLED", True)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.element_size() == 4 else t


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(_bits(a), _bits(b)), what


def _bn_params(C, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = (torch.rand(C, generator=g) + 0.5)
    gamma[5] = -0.75                      # a channel that BatchNorm flips
    beta = torch.randn(C, generator=g) * 0.25
    return gamma.cuda(), beta.cuda()


def _separate_fwd(z, gamma, beta, rm, rv, groups):
    """md2_bn_fwd_mask + md2_maxpool3s2_fwd on the raw ABI."""
    L = _lib.lib()
    B, C, H, W = z.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d, nbytes = bn_ops._desc((B * H * W, C, _lib.BN_RELU, EPS, MOM, groups))
    ws = bn_ops._workspace(z.device, nbytes)
    y = torch.empty_like(z, memory_format=CL)
    mask = torch.empty(z.numel() // 4, dtype=torch.uint8, device=z.device)
    stats = torch.empty(2, groups, C, device=z.device)
    st = _lib.stream(z.device)
    _lib.check(L.md2_bn_fwd_mask(ctypes.byref(d), z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None,
                                 rm.data_ptr(), rv.data_ptr(), y.data_ptr(), mask.data_ptr(), stats[0].data_ptr(),
                                 stats[1].data_ptr(), ws.data_ptr(), st), "md2_bn_fwd_mask")
    p = torch.empty((B, C, Ho, Wo), device=z.device, memory_format=CL)
    idx = torch.empty(B * Ho * Wo * C // 4, device=z.device, dtype=torch.int32)
    pd = _lib.PoolDesc(B, C, H, W, 0, 0)
    _lib.check(L.md2_maxpool3s2_fwd(ctypes.byref(pd), y.data_ptr(), p.data_ptr(), idx.data_ptr(), st),
               "md2_maxpool3s2_fwd")
    return p, idx, mask, y, stats[0], stats[1]


def _stem_z(shape, seed, nan=False):
    """A stem output quantised to multiples of 1/4 (window ties), one window of channel 9
    far below the mean (all negative after BatchNorm: a window of ReLU zeros)."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(shape, generator=g) * 4).round() / 4
    z[0, 9, 1:4, 3:6] = -16.0
    if nan:
        z[-1, 3, 2, 4] = float("nan")
    return z.cuda().contiguous(memory_format=CL)


@pytest.mark.parametrize("shape,groups", [((2, 64, 6, 10), 1), ((4, 64, 6, 10), 2), ((2, 64, 5, 9), 1)])
@pytest.mark.parametrize("need_y", [True, False])
@pytest.mark.parametrize("nan", [False, True])
def test_fused_forward_is_the_separate_launches(shape, groups, need_y, nan):
    z = _stem_z(shape, 11, nan)
    gamma, beta = _bn_params(shape[1], 5)
    rm0, rv0 = torch.zeros(shape[1], device="cuda"), torch.ones(shape[1], device="cuda")
    rm1, rv1 = rm0.clone(), rv0.clone()
    ref = _separate_fwd(z, gamma, beta, rm0, rv0, groups)
    L = _lib.lib()
    d, _ = bn_ops._desc((shape[0] * shape[2] * shape[3], shape[1], _lib.BN_RELU, EPS, MOM, groups))
    even = shape[2] % 2 == 0 and shape[3] % 2 == 0
    assert bool(L.md2_bn_pool_fwd_supported(ctypes.byref(d), shape[2], shape[3])) == even
    p, idx, mask, y, mean, invstd, _ = stem_ops.bn_relu_pool_fwd(z, gamma, beta, rm1, rv1, EPS, MOM, groups, need_y)
    if not nan:   # the cases hold what they are meant to: ties, and a window of zeros
        assert (ref[3][0, 9, 1:4, 3:6] == 0).all() and (ref[0] == 0).any()
        assert (ref[3] > 0).any() and ref[3][:, 5].ne(0).any()
    _same(p, ref[0], "pooled map")
    _same(idx, ref[1], "pool indices")
    _same(mask, ref[2], "ReLU mask")
    if need_y or not even:
        _same(y, ref[3], "y")
    else:
        assert y is None
    _same(mean, ref[4], "saved mean")
    _same(invstd, ref[5], "saved invstd")
    _same(rm1, rm0, "running mean")
    _same(rv1, rv0, "running var")


@pytest.mark.parametrize("xshape,groups", [((2, 3, 12, 20), 1),     # one partial 64-pixel segment per row
                                           ((1, 3, 4, 140), 1),     # output width 70: a full and a partial segment
                                           ((4, 6, 12, 20), 2),
                                           # 774 chunks in 387 K splits of two; split 193 spans both BatchNorm groups
                                           ((6, 6, 86, 260), 2)])
@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("w_cl", [True, False])
def test_fused_wgrad_is_the_separate_launches(xshape, groups, prefetch, w_cl):
    B, Cin, H, W = xshape
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(xshape, generator=gen).cuda().contiguous(memory_format=CL)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    z = (torch.randn(B, 64, Ho, Wo, generator=gen) * 2).cuda().contiguous(memory_format=CL)
    g = torch.randn(B, 64, Ho, Wo, generator=gen).cuda().contiguous(memory_format=CL)
    gamma, beta = _bn_params(64, 7)
    rm, rv = torch.zeros(64, device="cuda"), torch.ones(64, device="cuda")
    _, _, mask, _, mean, invstd = _separate_fwd(z, gamma, beta, rm, rv, groups)
    L = _lib.lib()
    d, nbytes = bn_ops._desc((B * Ho * Wo, 64, _lib.BN_RELU, EPS, MOM, groups))
    ws = bn_ops._workspace(z.device, nbytes)
    st = _lib.stream(z.device)
    flags = (_lib.STEM_WEIGHT_CL if w_cl else 0) | (_lib.STEM_PREFETCH if prefetch else 0)
    sd = _lib.StemDesc(B, Cin, H, W, flags)
    assert L.md2_stem_wgrad_bn_supported(ctypes.byref(sd))
    wfmt = CL if w_cl else torch.contiguous_format
    sws = torch.empty(L.md2_stem_wgrad_workspace_bytes(ctypes.byref(sd)), dtype=torch.uint8, device="cuda")

    # separate: md2_bn_bwd_mask writes gz, the default md2_stem_wgrad reads it
    gz = torch.empty_like(z, memory_format=CL)
    gg0, gb0 = torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
    _lib.check(L.md2_bn_bwd_mask(ctypes.byref(d), z.data_ptr(), mask.data_ptr(), g.data_ptr(), None, None,
                                 gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gz.data_ptr(), None,
                                 gg0.data_ptr(), gb0.data_ptr(), ws.data_ptr(), st), "md2_bn_bwd_mask")
    gw0 = torch.empty((64, Cin, 7, 7), device="cuda", memory_format=wfmt)
    sd0 = _lib.StemDesc(B, Cin, H, W, _lib.STEM_WEIGHT_CL if w_cl else 0)
    _lib.check(L.md2_stem_wgrad(ctypes.byref(sd0), x.data_ptr(), gz.data_ptr(), gw0.data_ptr(), sws.data_ptr(), st),
               "md2_stem_wgrad")

    # fused: the reductions, then the weight gradient on g, z and the mask
    gg1, gb1 = torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
    _lib.check(L.md2_bn_bwd_reduce_mask(ctypes.byref(d), z.data_ptr(), mask.data_ptr(), g.data_ptr(),
                                        gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gg1.data_ptr(),
                                        gb1.data_ptr(), ws.data_ptr(), st), "md2_bn_bwd_reduce_mask")
    coef = ws.data_ptr() + L.md2_bn_coef_offset(ctypes.byref(d))
    gw1 = torch.empty((64, Cin, 7, 7), device="cuda", memory_format=wfmt)
    _lib.check(L.md2_stem_wgrad_bn(ctypes.byref(sd), x.data_ptr(), g.data_ptr(), z.data_ptr(), mask.data_ptr(),
                                   mean.data_ptr(), coef, groups, gw1.data_ptr(), sws.data_ptr(), st),
               "md2_stem_wgrad_bn")
    assert gw0.abs().max() > 0
    _same(gw1, gw0, "dW")
    _same(gg1, gg0, "dgamma")
    _same(gb1, gb0, "dbeta")


def _encoder_run(enc, x, need_f0, weights, groups=1):
    """One forward + backward: (features, parameter gradients by name)."""
    enc.zero_grad(set_to_none=True)
    with bn_ops.bn_groups(groups):
        feats = enc.forward_prepared(x, need_f0=need_f0)
    loss = sum((f * w).sum() for f, w in zip(feats, weights) if f is not None)
    loss.backward()
    return feats, {n: p.grad for n, p in enc.named_parameters() if p.grad is not None}


def _encoder_case(num_input_images):
    torch.manual_seed(17)
    enc = ResnetEncoder(18, False, num_input_images=num_input_images).cuda().to(memory_format=CL).train()
    with torch.no_grad():
        enc.encoder.bn1.weight[5] = -0.75
    x = torch.randn(2, 3 * num_input_images, 32, 64, device="cuda").contiguous(memory_format=CL)
    shapes = [(2, 64, 16, 32), (2, 64, 8, 16), (2, 128, 4, 8), (2, 256, 2, 4), (2, 512, 1, 2)]
    weights = [torch.randn(s, device="cuda") for s in shapes]
    return enc, x, weights


def _check_encoder(got, ref, need_f0):
    (f1, g1), (f0, g0) = got, ref
    assert (f1[0] is None) == (not need_f0) and (f0[0] is None) == (not need_f0)
    for i, (a, b) in enumerate(zip(f1, f0)):
        if a is not None:
            _same(a.detach(), b.detach(), f"feature {i}")
    assert set(g1) == set(g0) and "encoder.conv1.weight" in g1 and "encoder.bn1.weight" in g1
    for n in g0:
        _same(g1[n], g0[n], n)


def test_encoder_fused_is_unfused(monkeypatch):
    """ResnetEncoder(18), depth-encoder form: every feature (features[0] included) and every
    parameter gradient, fused stem vs MD2_STEM_FUSE=0."""
    monkeypatch.setattr(conv_ops, "AUTOTUNE", False)
    enc, x, weights = _encoder_case(1)
    ref_enc = copy.deepcopy(enc)
    monkeypatch.setattr(stem_ops, "FUSE", False)
    ref = _encoder_run(ref_enc, x, True, weights)
    assert "StemBNPool" not in type(ref[0][1].grad_fn).__name__
    monkeypatch.setattr(stem_ops, "FUSE", True)
    got = _encoder_run(enc, x, True, weights)
    _check_encoder(got, ref, True)
    _same(enc.encoder.bn1.running_var, ref_enc.encoder.bn1.running_var, "running var")


def test_pose_encoder_fused_captured_is_unfused(monkeypatch):
    """The pose-encoder form (two input images, one BatchNorm group per image as the
    trainer's batched frame pairs, need_f0=False: features[0] is None and y is never made),
    eager and captured in a hipGraph replayed twice, vs MD2_STEM_FUSE=0."""
    monkeypatch.setattr(conv_ops, "AUTOTUNE", False)
    enc, x, weights = _encoder_case(2)
    ref_enc = copy.deepcopy(enc)
    monkeypatch.setattr(stem_ops, "FUSE", False)
    ref = _encoder_run(ref_enc, x, False, weights, groups=2)
    monkeypatch.setattr(stem_ops, "FUSE", True)

    # every backward of `enc` runs on the capture's stream, the eager one included (it is
    # the capture's warm-up too): a parameter's AccumulateGrad node keeps the stream of its
    # first backward (Trainer._capture), and one left on the default stream would pull that
    # stream into the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _encoder_run(enc, x, False, weights, groups=2)
    torch.cuda.current_stream().wait_stream(side)
    _check_encoder(got, ref, False)
    del got
    enc.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        feats, grads = _encoder_run(enc, x, False, weights, groups=2)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _check_encoder((feats, grads), ref, False)
