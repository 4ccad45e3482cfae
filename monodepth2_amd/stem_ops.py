"""The ResNet stem convolution (conv1: 7x7, stride 2, padding 3, C -> 64, no bias) on
split-bf16 MFMA (csrc/stem.hip, ABI `md2_stem_*`): forward and weight gradient.

The stem reads the normalised frames, which are data: its backward is the weight
gradient alone, MIOpen's igemm_wrw at ~125 us (C=3, depth encoder, B=12) and ~430 us
(C=6, pose encoder, B=24) per step at 192x640.  stem_x6_wgrad_tr_kernel (f32-class:
three exact bf16 planes, six products; the window taps read from the staged rows with
transposing LDS reads) runs them in ~0.082 / ~0.21 ms including its split reduction
(tools/stem_bench.py; the earlier im2col-build kernel: ~0.10 / ~0.40 ms).  The forward
(MIOpen's igemm_fwd: 89 / 334 us) runs on stem_x6_fwd_kernel for C = 3 / 6 (the input
windows read straight from the NHWC rows as MFMA fragments, FWD_ENABLED).  Same
parameter (the torchvision `conv1.weight`), same semantics; any other case (an input
that needs a gradient, bf16, NCHW inputs, a CPU tensor) runs the module itself.

stem_bn_pool runs the whole stem chain conv1 -> bn1 -> ReLU -> max-pool as one autograd
node whose BatchNorm elementwise passes are folded into the pool (forward) and into the
weight gradient (backward): md2_bn_pool_fwd, md2_bn_bwd_reduce_mask, md2_stem_wgrad_bn.
"""
from __future__ import annotations

import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

_CL = torch.channels_last
ENABLED = True       # the x6 weight gradient (tests flip it to compare with MIOpen)
FWD_ENABLED = os.environ.get("MD2_STEM_FWD", "1") != "0"   # the x6 forward (C = 3 / 6); 0: MIOpen's (A/B)
# bf16 autocast: the weight gradient on md2_stem_wgrad (deterministic) instead of MIOpen's bf16 one
BF16_ENABLED = os.environ.get("MD2_CONV_BF16", "1") != "0"


def _fwd(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """conv2d(x, weight, stride 2, padding 3) on md2_stem_fwd, or MIOpen's forward."""
    B, C, H, W = x.shape
    if not (FWD_ENABLED and C in (3, 6)):
        return F.conv2d(x, weight, None, 2, 3)
    w_cl = weight.is_contiguous(memory_format=_CL)
    if not (w_cl or weight.is_contiguous()):
        weight = weight.contiguous()
    d = _lib.StemDesc(B, C, H, W, _lib.STEM_WEIGHT_CL if w_cl else 0)
    y = torch.empty((B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1), device=x.device, dtype=torch.float32,
                    memory_format=_CL)
    rc = _lib.lib().md2_stem_fwd(ctypes.byref(d), x.data_ptr(), weight.data_ptr(), y.data_ptr(), _lib.stream(x.device))
    _lib.check(rc, "md2_stem_fwd")
    return y


def _fwd_bf16(xb: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """The bf16 autocast stem convolution on md2_stem_fwd (MD2_STEM_BF16, ABI 23): bf16 x,
    the weight rounded to bf16 in the kernel, fp32 accumulation, bf16 y (C = 3 / 6)."""
    B, C, H, W = xb.shape
    w_cl = weight.is_contiguous(memory_format=_CL)
    if not (w_cl or weight.is_contiguous()):
        weight = weight.contiguous()
    d = _lib.StemDesc(B, C, H, W, (_lib.STEM_WEIGHT_CL if w_cl else 0) | _lib.STEM_BF16)
    y = torch.empty((B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1), device=xb.device, dtype=torch.bfloat16,
                    memory_format=_CL)
    _lib.check(_lib.lib().md2_stem_fwd(ctypes.byref(d), xb.data_ptr(), weight.data_ptr(), y.data_ptr(),
                                       _lib.stream(xb.device)), "md2_stem_fwd")
    return y


_FWD_BF16 = os.environ.get("MD2_STEM_FWD_BF16", "1") != "0"   # A/B knob: 0 = MIOpen's bf16 forward


class _StemConv(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x)
        ctx.w_cl = weight.is_contiguous(memory_format=_CL)
        ctx.w_shape = weight.shape
        return _fwd(x, weight)

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gy = gy.contiguous(memory_format=_CL)
        B, C, H, W = x.shape
        d = _lib.StemDesc(B, C, H, W, _lib.STEM_WEIGHT_CL if ctx.w_cl else 0)
        gw = torch.empty(ctx.w_shape, device=x.device, dtype=torch.float32,
                         memory_format=_CL if ctx.w_cl else torch.contiguous_format)
        L = _lib.lib()
        ws = torch.empty(L.md2_stem_wgrad_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device=x.device)
        rc = L.md2_stem_wgrad(ctypes.byref(d), x.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(),
                              _lib.stream(x.device))
        _lib.check(rc, "md2_stem_wgrad")
        return None, gw


_WGRAD_BF16 = os.environ.get("MD2_STEM_WGRAD_BF16", "1") != "0"   # A/B knob: 0 = fp32 copies of the operands


class _StemConvBF16(torch.autograd.Function):
    """The stem under bf16 autocast (config C5): the forward is autocast's arithmetic — x
    and the weight cast to bf16, fp32 accumulation, a bf16 output — on md2_stem_fwd's bf16
    form (C = 3 / 6; else MIOpen's bf16 convolution), and the weight gradient, which MIOpen
    computes non-deterministically in bf16, runs on md2_stem_wgrad (fixed-order reduction)
    over the bf16 operands themselves (MD2_STEM_BF16; C = 9: their exact fp32 values), then
    rounded to bf16 as the autocast cast's backward would hand it to the parameter."""

    @staticmethod
    def forward(ctx, x, weight):
        xb = x.to(torch.bfloat16)
        ctx.save_for_backward(xb)
        ctx.w_cl = weight.is_contiguous(memory_format=_CL)
        ctx.w_shape = weight.shape
        if _FWD_BF16 and FWD_ENABLED and xb.shape[1] in (3, 6) and xb.is_contiguous(memory_format=_CL):
            return _fwd_bf16(xb, weight)
        with torch.autocast("cuda", enabled=False):
            return F.conv2d(xb, weight.to(torch.bfloat16), None, 2, 3)

    @staticmethod
    def backward(ctx, gy):
        xb, = ctx.saved_tensors
        B, C, H, W = xb.shape
        flags = _lib.STEM_WEIGHT_CL if ctx.w_cl else 0
        if C in (3, 6) and gy.dtype == torch.bfloat16 and _WGRAD_BF16:
            # the bf16 operands as they are (MD2_STEM_BF16, ABI 23): one MFMA per fragment
            # pair instead of six with five zero planes, no fp32 copies — bitwise the same
            # sums (the zero planes add exact zeros; tests/test_stem_gpu.py)
            x = xb.contiguous(memory_format=_CL)
            gy = gy.contiguous(memory_format=_CL)
            flags |= _lib.STEM_BF16
        else:
            x = xb.float().contiguous(memory_format=_CL)
            gy = gy.float().contiguous(memory_format=_CL)
        d = _lib.StemDesc(B, C, H, W, flags)
        gw = torch.empty(ctx.w_shape, device=x.device, dtype=torch.float32,
                         memory_format=_CL if ctx.w_cl else torch.contiguous_format)
        L = _lib.lib()
        ws = torch.empty(L.md2_stem_wgrad_workspace_bytes(ctypes.byref(d)), dtype=torch.uint8, device=x.device)
        _lib.check(L.md2_stem_wgrad(ctypes.byref(d), x.data_ptr(), gy.data_ptr(), gw.data_ptr(), ws.data_ptr(),
                                    _lib.stream(x.device)), "md2_stem_wgrad")
        return None, gw.to(torch.bfloat16).to(torch.float32)


# A/B knobs of the fused stem chain (stem_bn_pool): MD2_STEM_FUSE=0 runs the separate
# stem_conv / bn_act / max_pool launches; MD2_STEM_FUSE_FWD=0 / MD2_STEM_FUSE_WGRAD=0 keep
# the separate launches of the forward half / the backward half alone
FUSE = os.environ.get("MD2_STEM_FUSE", "1") != "0"
FUSE_FWD = os.environ.get("MD2_STEM_FUSE_FWD", "1") != "0"
FUSE_WGRAD = os.environ.get("MD2_STEM_FUSE_WGRAD", "1") != "0"


def bn_relu_pool_fwd(z, gamma, beta, running_mean, running_var, eps: float, momentum: float, groups: int,
                     need_y: bool):
    """pool(relu(bn(z))) for a training-mode BatchNorm (per chunk with groups > 1) and
    MaxPool2d(3, 2, 1) on an fp32 channels_last z: (pooled map, pool index words, ReLU mask,
    y, saved mean, saved invstd, BatchNorm desc key).  On md2_bn_pool_fwd (one pass over
    z; y = relu(bn(z)) is None unless need_y) for even sizes, else on md2_bn_fwd_mask +
    md2_maxpool3s2_fwd (y always made).  The running statistics are updated in place."""
    from . import bn_ops
    B, C, H, W = z.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    key = (B * H * W, C, _lib.BN_RELU, eps, momentum, groups)
    d, nbytes = bn_ops._desc(key)
    L = _lib.lib()
    ws = bn_ops._workspace(z.device, nbytes)
    stats = torch.empty(2, groups, C, device=z.device)   # saved mean, invstd
    mean, invstd = stats[0], stats[1]
    mask = torch.empty(z.numel() // 4, dtype=torch.uint8, device=z.device)
    p = torch.empty((B, C, Ho, Wo), device=z.device, dtype=z.dtype, memory_format=_CL)
    idx = torch.empty(B * Ho * Wo * C // 4, device=z.device, dtype=torch.int32)
    stream = _lib.stream(z.device)
    rm = running_mean.data_ptr() if running_mean is not None else None
    rv = running_var.data_ptr() if running_var is not None else None
    if FUSE_FWD and L.md2_bn_pool_fwd_supported(ctypes.byref(d), H, W):
        y = torch.empty_like(z, memory_format=_CL) if need_y else None
        _lib.check(L.md2_bn_pool_fwd(ctypes.byref(d), H, W, z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm, rv,
                                     y.data_ptr() if y is not None else None, mask.data_ptr(), p.data_ptr(),
                                     idx.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), stream),
                   "md2_bn_pool_fwd")
    else:   # odd sizes: the two launches
        y = torch.empty_like(z, memory_format=_CL)
        _lib.check(L.md2_bn_fwd_mask(ctypes.byref(d), z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, rm, rv,
                                     y.data_ptr(), mask.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                     ws.data_ptr(), stream), "md2_bn_fwd_mask")
        pd = _lib.PoolDesc(B, C, H, W, 0, 0)
        _lib.check(L.md2_maxpool3s2_fwd(ctypes.byref(pd), y.data_ptr(), p.data_ptr(), idx.data_ptr(), stream),
                   "md2_maxpool3s2_fwd")
    return p, idx, mask, y, mean, invstd, key


class _StemBNPool(torch.autograd.Function):
    """conv1 -> bn1 -> ReLU -> MaxPool2d(3, 2, 1) of the ResNet stem as one autograd node
    (fp32, channels_last).  Outputs (p, p'[, y]): the pooled map, a view of it for its
    second consumer (the first block's shortcut) and, with need_f0, y = relu(bn1(conv1(x)))
    for the decoder skip; all their gradients meet in this backward's pool gather, as
    with max_pool_3x3s2_with_alias.

    Forward: md2_bn_pool_fwd reads z = conv1(x) once and writes the pooled map, the pool
    indices, the ReLU mask and, only with need_f0, y (the separate launches write y and
    read it back for the pool).  Backward: the BatchNorm reductions (dγ, dβ, the dx
    coefficients) and then md2_stem_wgrad_bn, which forms the stem output's gradient on
    load; it is never written.  The coefficients live in this stream's BatchNorm
    workspace, so the reductions and the weight gradient are issued here back to back.
    Every output is bitwise what the separate launches give (tests/test_stem_fused_gpu.py)."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, eps: float, momentum: float, groups: int,
                need_f0: bool):
        z = _fwd(x, weight)
        p, idx, mask, y, mean, invstd, key = bn_relu_pool_fwd(z, gamma, beta, running_mean, running_var, eps,
                                                              momentum, groups, need_f0)
        ctx.save_for_backward(x, z, mask, idx, gamma, mean, invstd)
        ctx.bn_key = key
        ctx.w_cl = weight.is_contiguous(memory_format=_CL)
        ctx.w_shape = weight.shape
        ctx.set_materialize_grads(False)   # an unused output brings None, not a zero tensor
        return (p, p.view_as(p)) + ((y,) if need_f0 else ())

    @staticmethod
    def backward(ctx, gp, gp2, gf0=None):
        from . import bn_ops
        x, z, mask, idx, gamma, mean, invstd = ctx.saved_tensors
        if gp is None:
            gp, gp2 = gp2, None
        if gp is None and gf0 is None:
            return (None,) * 10
        L = _lib.lib()
        B, C, H, W = z.shape
        stream = _lib.stream(z.device)
        if gf0 is not None:
            gf0 = gf0.to(z.dtype).contiguous(memory_format=_CL)
        if gp is None:   # only y reached the loss: the pool adds nothing
            g = gf0
        else:
            gp = gp.to(z.dtype).contiguous(memory_format=_CL)
            if gp2 is not None:
                gp2 = gp2.to(z.dtype).contiguous(memory_format=_CL)
            g = torch.empty_like(z, memory_format=_CL)
            pd = _lib.PoolDesc(B, C, H, W, 0, 0)
            _lib.check(L.md2_maxpool3s2_bwd_multi(ctypes.byref(pd), idx.data_ptr(), gp.data_ptr(),
                                                  gp2.data_ptr() if gp2 is not None else None,
                                                  gf0.data_ptr() if gf0 is not None else None, g.data_ptr(), stream),
                       "md2_maxpool3s2_bwd_multi")
        d, nbytes = bn_ops._desc(ctx.bn_key)
        ws = bn_ops._workspace(z.device, nbytes)
        ggamma = torch.empty_like(gamma)
        gbeta = torch.empty_like(gamma)
        xb, xc, xh, xw = x.shape
        sd = _lib.StemDesc(xb, xc, xh, xw, _lib.STEM_WEIGHT_CL if ctx.w_cl else 0)
        gw = torch.empty(ctx.w_shape, device=x.device, dtype=torch.float32,
                         memory_format=_CL if ctx.w_cl else torch.contiguous_format)
        sws = torch.empty(L.md2_stem_wgrad_workspace_bytes(ctypes.byref(sd)), dtype=torch.uint8, device=x.device)
        if FUSE_WGRAD and L.md2_stem_wgrad_bn_supported(ctypes.byref(sd)):
            _lib.check(L.md2_bn_bwd_reduce_mask(ctypes.byref(d), z.data_ptr(), mask.data_ptr(), g.data_ptr(),
                                                gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                                ggamma.data_ptr(), gbeta.data_ptr(), ws.data_ptr(), stream),
                       "md2_bn_bwd_reduce_mask")
            coef = ws.data_ptr() + L.md2_bn_coef_offset(ctypes.byref(d))
            _lib.check(L.md2_stem_wgrad_bn(ctypes.byref(sd), x.data_ptr(), g.data_ptr(), z.data_ptr(), mask.data_ptr(),
                                           mean.data_ptr(), coef, ctx.bn_key[5], gw.data_ptr(), sws.data_ptr(),
                                           stream), "md2_stem_wgrad_bn")
        else:
            gz = torch.empty_like(z, memory_format=_CL)
            _lib.check(L.md2_bn_bwd_mask(ctypes.byref(d), z.data_ptr(), mask.data_ptr(), g.data_ptr(), None, None,
                                         gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gz.data_ptr(), None,
                                         ggamma.data_ptr(), gbeta.data_ptr(), ws.data_ptr(), stream),
                       "md2_bn_bwd_mask")
            _lib.check(L.md2_stem_wgrad(ctypes.byref(sd), x.data_ptr(), gz.data_ptr(), gw.data_ptr(), sws.data_ptr(),
                                        stream), "md2_stem_wgrad")
        return None, gw, ggamma, gbeta, None, None, None, None, None, None


def stem_bn_pool(conv: nn.Conv2d, bn: nn.BatchNorm2d, pool: nn.MaxPool2d, x: torch.Tensor, need_f0: bool = True):
    """The ResNet stem chain pool(relu(bn(conv(x)))): returns (p, p', f0) — the pooled map,
    a view of it for its second consumer, and f0 = relu(bn(conv(x))) for the decoder skip
    (None without need_f0).  Training-mode fp32 channels_last GPU inputs run as one
    autograd node on the fused kernels (_StemBNPool); anything else, and MD2_STEM_FUSE=0,
    as stem_conv -> bn_act -> max_pool_3x3s2_with_alias."""
    from . import bn_ops
    groups = bn_ops._GROUPS if bn.training else 1
    if (FUSE and ENABLED and FWD_ENABLED and bn_ops.ENABLED and supports_stem(conv, x) and x.shape[1] in (3, 6)
            and torch.is_grad_enabled() and conv.weight.requires_grad
            and bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None
            and bn.weight.dtype == torch.float32 and x.shape[0] % groups == 0
            and x.shape[0] * ((x.shape[2] - 1) // 2 + 1) * ((x.shape[3] - 1) // 2 + 1) * 16 // groups < 2 ** 31
            and bn_ops._pool_geometry_ok(pool) and bn_ops._ALIAS_SUM):
        if bn.num_batches_tracked is not None:   # nn.BatchNorm2d counts training batches
            bn.num_batches_tracked.add_(groups)
        out = _StemBNPool.apply(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                                bn.momentum, groups, need_f0)
        return (out[0], out[1], out[2] if need_f0 else None)
    f0 = bn_ops.bn_act(bn, stem_conv(conv, x))
    p, ps, f0 = bn_ops.max_pool_3x3s2_with_alias(pool, f0, out_alias=True)
    return p, ps, (f0 if need_f0 else None)


def supports_stem_bf16(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    from .conv_ops import _bf16_autocast
    return (BF16_ENABLED and x.is_cuda and x.dtype == torch.float32 and conv.weight.dtype == torch.float32
            and not x.requires_grad and x.dim() == 4 and x.shape[1] in (3, 6, 9)
            and x.is_contiguous(memory_format=_CL) and conv.out_channels == 64
            and tuple(conv.kernel_size) == (7, 7) and tuple(conv.stride) == (2, 2) and tuple(conv.padding) == (3, 3)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.padding_mode == "zeros" and _bf16_autocast() and x.numel() < 2 ** 31)


def supports_stem(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and conv.weight.dtype == torch.float32 and not x.requires_grad
            and x.dim() == 4 and x.shape[1] in (3, 6, 9) and x.is_contiguous(memory_format=_CL)
            and conv.out_channels == 64 and tuple(conv.kernel_size) == (7, 7) and tuple(conv.stride) == (2, 2)
            and tuple(conv.padding) == (3, 3) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and conv.bias is None and conv.padding_mode == "zeros" and not torch.is_autocast_enabled()
            and x.numel() < 2 ** 31)


def stem_conv(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """conv(x) for the encoder's stem; the weight gradient runs on md2_stem_wgrad when
    supports_stem(conv, x), else the module runs as is."""
    if ENABLED and supports_stem(conv, x):
        if torch.is_grad_enabled() and conv.weight.requires_grad:
            return _StemConv.apply(x, conv.weight)
        return _fwd(x, conv.weight.detach())
    if ENABLED and torch.is_grad_enabled() and conv.weight.requires_grad and supports_stem_bf16(conv, x):
        return _StemConvBF16.apply(x, conv.weight)
    return conv(x)
