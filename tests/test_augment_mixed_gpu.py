"""Mixed decoded sizes in one batch (md2_aug_plan_create_mixed / md2_aug_run_mixed,
augment.GpuAugmentMixed) vs the PIL-pinned oracle and vs single-size plans.  The bar is
bit-exact, per item: a batch that mixes sizes gives every item the bits it gets alone.

The feed is 24 x 72 with 3 scales (a partial 64 x 16 tile both ways: 72 = 64 + 8,
24 = 16 + 8), frame ids [0, -1, 1], and six items whose scale-0 routes are
(window sizes are 2 * ceil(3 * max(in / out, 1)) + 1, columns / rows):

    item 0  47 x 139   fused kernel, 13 / 13 taps
    item 1  46 x 137   fused 13 / 13 too, but other tables: a class of its own
    item 2  47 x 139   shares item 0's class (one launch covers both)
    item 3  30 x 100   fused 11 / 9
    item 4  15 x 40    up-scaling: fused 7 / 7
    item 5  80 x 250   23 / 21 taps, above 13: the two-pass route (and its mean pass)
"""
import ctypes
import math
import random

import numpy as np
import pytest
import torch

from oracle import augment_oracle as A

pytestmark = pytest.mark.gpu

H, W, S = 24, 72, 3
SIZES = [(47, 139), (46, 137), (47, 139), (30, 100), (15, 40), (80, 250)]
ROUTES = [(13, 13), (13, 13), (13, 13), (11, 9), (7, 7), (23, 21)]   # (columns, rows)
FRAME_IDS = [0, -1, 1]


def _ksize(n_in, n_out):
    return int(math.ceil(3.0 * max(n_in / n_out, 1.0))) * 2 + 1


def _image(rng, h, w):
    """A textured uint8 frame (smooth + noise, like a camera image)."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.zeros((h, w, 3))
    for _ in range(6):
        k = rng.uniform(0.02, 0.3, 2)
        base += rng.uniform(20, 60) * np.sin(k[0] * xx + k[1] * yy + rng.uniform(0, 6.3))[..., None] \
            * rng.uniform(0.3, 1.0, 3)
    base += 128 + rng.normal(0, 12, base.shape)
    return np.clip(base, 0, 255).astype(np.uint8)


def _draws():
    from monodepth2_amd.augment import ItemDraw, draw_item
    return [ItemDraw(True, True, 1.15, 0.83, 1.07, -0.09, [1, 3, 0, 2]),   # contrast first
            ItemDraw(True, False, 0.81, 1.19, 0.92, 0.06, [3, 2, 1, 0]),   # contrast after hue+sat
            ItemDraw(False, True),
            ItemDraw(True, True, 1.2, 0.85, 0.8, 0.1, [0, 1, 2, 3]),
            draw_item(random.Random(5)),
            ItemDraw(True, True, 0.9, 1.1, 1.2, -0.02, [2, 1, 3, 0])]


def _oracle(img, d):
    jit = (d.order, d.brightness, d.contrast, d.saturation, d.hue) if d.do_color_aug else None
    return A.preprocess(img, H, W, S, flip=d.do_flip, jitter=jit)


@pytest.fixture(scope="module")
def case():
    """Frames, draws and the oracle's outputs, computed once and left unchanged."""
    rng = np.random.default_rng(7)
    frames = [[_image(rng, h, w) for (h, w) in SIZES] for _ in FRAME_IDS]   # [f][b]
    draws = _draws()
    want = [[_oracle(frames[f][b], draws[b]) for b in range(len(SIZES))] for f in range(len(FRAME_IDS))]
    return frames, draws, want


def _run(aug, frames, draws, sides=None, order=None, align=256, lead=0):
    """One mixed call on items `order` (default all), packed with `align`-byte offsets
    after `lead` unused bytes; returns the input dict."""
    from monodepth2_amd.augment import pack_ragged
    order = list(range(len(frames[0]))) if order is None else order
    sel = [[fr[b] for b in order] for fr in frames]
    buf, offs, sizes = pack_ragged(sel, align=align)
    if lead:
        buf = np.concatenate([np.zeros(lead, np.uint8), buf])
        offs = [o + lead for o in offs]
    out = aug(torch.from_numpy(buf).cuda(), sizes, offs, [draws[b] for b in order], sides)
    torch.cuda.synchronize()
    return out


def test_routes_are_the_documented_ones():
    for (h, w), (kx, ky) in zip(SIZES, ROUTES):
        assert (_ksize(w, W), _ksize(h, H)) == (kx, ky), (h, w)


def test_mixed_batch_bit_exact(case):
    """(1) every color / color_aug value equals the oracle's for that item; (2) and a
    single-size GpuAugment run on the item alone; (3) color_src8 == pack_rgbx."""
    from monodepth2_amd.augment import GpuAugment, GpuAugmentMixed
    from monodepth2_amd.data import pack_rgbx
    frames, draws, want = case
    B = len(SIZES)
    aug = GpuAugmentMixed(H, W, FRAME_IDS, B, S, sizes=sorted(set(SIZES)))
    out = _run(aug, frames, draws)
    assert aug.rebuilds == 0
    for fi, fid in enumerate(FRAME_IDS):
        for b in range(B):
            color, caug = want[fi][b]
            for s in range(S):
                got = out[("color", fid, s)][b].cpu().numpy()
                gaug = out[("color_aug", fid, s)][b].cpu().numpy()
                assert np.array_equal(got, color[s]), (fid, b, s, int((got != color[s]).sum()))
                assert np.array_equal(gaug, caug[s]), (fid, b, s, draws[b], int((gaug != caug[s]).sum()))
    assert torch.equal(out["color_src8"], pack_rgbx([out[("color", f, 0)] for f in FRAME_IDS[1:]]))
    K, inv_K = out[("K", 1)], out[("inv_K", 1)]
    assert K.shape == (B, 4, 4) and float(K[0, 0, 0]) == pytest.approx(0.58 * 36)
    assert inv_K.shape == (B, 4, 4)
    for b, (h, w) in enumerate(SIZES):
        one = GpuAugment(H, W, h, w, FRAME_IDS, 1, S)
        alone = one(torch.from_numpy(np.stack([fr[b] for fr in frames])[:, None]).cuda(), [draws[b]])
        torch.cuda.synchronize()
        for fid in FRAME_IDS:
            for s in range(S):
                for key in ("color", "color_aug"):
                    assert torch.equal(out[(key, fid, s)][b], alone[(key, fid, s)][0]), (key, fid, s, b)
        assert torch.equal(out["color_src8"][:, b], alone["color_src8"][:, 0]), b


def test_item_order_and_offsets_do_not_change_the_bits(case):
    """(4) items listed in another order, frames at other (16-aligned) offsets."""
    from monodepth2_amd.augment import GpuAugmentMixed
    frames, draws, _ = case
    B = len(SIZES)
    aug = GpuAugmentMixed(H, W, FRAME_IDS, B, S, sizes=SIZES)
    a = _run(aug, frames, draws)
    order = [5, 2, 4, 0, 3, 1]
    b = _run(aug, frames, draws, order=order, align=16, lead=48)
    for k in a:
        if isinstance(k, tuple) and k[0] in ("color", "color_aug"):
            for j, src in enumerate(order):
                assert torch.equal(b[k][j], a[k][src]), (k, j, src)
    for j, src in enumerate(order):
        assert torch.equal(b["color_src8"][:, j], a["color_src8"][:, src])


@pytest.mark.parametrize("order", [[0, 5, 3], [5]])
def test_odd_batch_sizes(case, order):
    """An item record is 20 bytes, so with an odd number of items the 64-bit frame offsets
    staged behind the records need their own alignment: batches of 3 and of 1."""
    from monodepth2_amd.augment import GpuAugmentMixed
    frames, draws, want = case
    aug = GpuAugmentMixed(H, W, FRAME_IDS, len(order), S, sizes=SIZES)
    for out in (_run(aug, frames, draws, order=order), _run(aug, frames, draws, order=order, align=16, lead=16)):
        for fi, fid in enumerate(FRAME_IDS):
            for j, b in enumerate(order):
                for s in range(S):
                    assert np.array_equal(out[("color", fid, s)][j].cpu().numpy(), want[fi][b][0][s]), (fid, b, s)
                    assert np.array_equal(out[("color_aug", fid, s)][j].cpu().numpy(), want[fi][b][1][s]), (fid, b, s)


def test_repeated_calls_and_streams(case):
    """(5) calls in a row on one plan (past the staging ring's length, so slots are
    reused) and a call on a second stream are bit-equal."""
    from monodepth2_amd.augment import GpuAugmentMixed, pack_ragged
    frames, draws, _ = case
    aug = GpuAugmentMixed(H, W, FRAME_IDS, len(SIZES), S, sizes=SIZES)
    buf, offs, sizes = pack_ragged(frames)
    dev = torch.from_numpy(buf).cuda()
    outs = [aug(dev, sizes, offs, draws) for _ in range(6)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs.append(aug(dev, sizes, offs, draws))
    torch.cuda.synchronize()
    for o in outs[1:]:
        for k in outs[0]:
            assert torch.equal(outs[0][k], o[k]), k


def test_stereo_pair_and_sides():
    from monodepth2_amd.augment import GpuAugmentMixed, ItemDraw
    rng = np.random.default_rng(11)
    sizes = [(47, 139), (30, 100)]
    ids = [0, "s"]
    frames = [[_image(rng, h, w) for (h, w) in sizes] for _ in ids]
    draws = [ItemDraw(True, True, 1.2, 1.2, 0.8, 0.1, [0, 1, 2, 3]), ItemDraw(False, False)]
    aug = GpuAugmentMixed(H, W, ids, 2, S)
    out = _run(aug, frames, draws, sides=["l", "r"])
    for fi, fid in enumerate(ids):
        for b in range(2):
            color, caug = _oracle(frames[fi][b], draws[b])
            for s in range(S):
                assert np.array_equal(out[("color", fid, s)][b].cpu().numpy(), color[s]), (fid, b, s)
                assert np.array_equal(out[("color_aug", fid, s)][b].cpu().numpy(), caug[s]), (fid, b, s)
    # mono_dataset.py:192-198: side_sign * baseline_sign * 0.1
    T = out["stereo_T"].cpu()
    assert float(T[0, 0, 3]) == pytest.approx(0.1) and float(T[1, 0, 3]) == pytest.approx(0.1)
    T = _run(aug, frames, draws, sides=["r", "l"])["stereo_T"].cpu()
    assert float(T[0, 0, 3]) == pytest.approx(-0.1) and float(T[1, 0, 3]) == pytest.approx(-0.1)
    with pytest.raises(ValueError, match="side"):
        _run(aug, frames, draws, sides=None)


def test_unknown_size_rebuilds_the_plan(case):
    from monodepth2_amd.augment import MAX_SIZES, GpuAugmentMixed
    frames, draws, want = case
    aug = GpuAugmentMixed(H, W, FRAME_IDS, 2, S, sizes=[(47, 139)])
    out = _run(aug, frames, draws, order=[0, 1])      # 46 x 137 is not in the plan
    assert aug.rebuilds == 1 and aug.sizes == [(47, 139), (46, 137)]
    out2 = _run(aug, frames, draws, order=[5, 0])     # nor is 80 x 250
    assert aug.rebuilds == 2
    for fi, fid in enumerate(FRAME_IDS):
        for s in range(S):
            for j, b in enumerate([0, 1]):
                assert np.array_equal(out[("color_aug", fid, s)][j].cpu().numpy(), want[fi][b][1][s]), (fid, s, b)
            for j, b in enumerate([5, 0]):
                assert np.array_equal(out2[("color_aug", fid, s)][j].cpu().numpy(), want[fi][b][1][s]), (fid, s, b)
    with pytest.raises(ValueError, match="at most 16"):
        GpuAugmentMixed(H, W, FRAME_IDS, 2, S, sizes=[(40 + i, 100) for i in range(MAX_SIZES + 1)])


def test_abi_refusals_without_a_launch():
    from monodepth2_amd import _lib
    L = _lib.lib()
    F, B = 2, 2
    desc = _lib.AugDesc(B, F, 0, 0, H, W, S, 0)
    sizes = (ctypes.c_int32 * 4)(47, 139, 30, 100)
    many = (ctypes.c_int32 * 34)(*([40, 100] * 17))
    for n, arr in ((0, sizes), (17, many)):
        assert not L.md2_aug_plan_create_mixed(ctypes.byref(desc), arr, n)
        assert b"num_sizes" in L.md2_last_error()
    assert not L.md2_aug_plan_create_mixed(ctypes.byref(desc), None, 2)
    plan = L.md2_aug_plan_create_mixed(ctypes.byref(desc), sizes, 2)
    assert plan
    try:
        per = 47 * 139 * 3
        step = (per + 255) // 256 * 256
        total = 4 * step
        buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
        color = [torch.empty(F, B, 3, H >> s, W >> s, device="cuda") for s in range(S)]
        caug = [torch.empty_like(c) for c in color]
        cp = (ctypes.c_void_p * S)(*[t.data_ptr() for t in color])
        ap = (ctypes.c_void_p * S)(*[t.data_ptr() for t in caug])
        items = (_lib.AugItem * B)()
        for it in items:
            for k in range(4):
                it.order[k] = k
        stream = _lib.stream(torch.device("cuda", torch.cuda.current_device()))

        def call(cls, offs, total_bytes=total, base=buf.data_ptr(), its=items):
            return L.md2_aug_run_mixed(plan, base, total_bytes, (ctypes.c_int32 * B)(*cls),
                                       (ctypes.c_uint64 * (F * B))(*offs), ctypes.byref(its), cp, ap, None, stream)

        good = [0, step, 2 * step, 3 * step]
        assert call([0, 2], good) == -1 and b"size class" in L.md2_last_error()
        assert call([0, -1], good) == -1 and b"size class" in L.md2_last_error()
        assert call([0, 0], [0, step + 8, 2 * step, 3 * step]) == -1 and b"multiple of 16" in L.md2_last_error()
        assert call([0, 0], [0, step, 2 * step, total]) == -1 and b"total_bytes" in L.md2_last_error()
        assert call([0, 0], good, total_bytes=3 * step + per - 1) == -1 and b"total_bytes" in L.md2_last_error()
        assert call([0, 0], good, base=None) == -1 and b"NULL" in L.md2_last_error()
        bad = (_lib.AugItem * B)()
        assert call([0, 0], good, its=bad) == -1 and b"permutation" in L.md2_last_error()
        # a mixed plan refuses the single-size entry point, and the other way round
        assert L.md2_aug_run2(plan, buf.data_ptr(), ctypes.byref(items), cp, ap, None, stream) == -1
        single_desc = _lib.AugDesc(B, F, 47, 139, H, W, S, 0)
        single = L.md2_aug_plan_create(ctypes.byref(single_desc))
        assert single
        try:
            assert L.md2_aug_run_mixed(single, buf.data_ptr(), total, (ctypes.c_int32 * B)(0, 0),
                                       (ctypes.c_uint64 * (F * B))(*good), ctypes.byref(items), cp, ap, None,
                                       stream) == -1
            assert b"mixed-size plan" in L.md2_last_error()
        finally:
            L.md2_aug_plan_destroy(single)
        # the exact fit is accepted
        assert call([0, 1], good, total_bytes=3 * step + 30 * 100 * 3) == 0
        torch.cuda.synchronize()
    finally:
        L.md2_aug_plan_destroy(plan)
