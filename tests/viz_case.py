"""The yardstick of the disparity-picture tests: a numpy restatement of md2_disp_colorize
(include/md2hot.h; the reference's test_simple.py:136-155) in the kernel's written order —
the fp32 bilinear resize, the order-preserving keys, numpy's `linear` percentile in fp32,
the minimum, matplotlib's Normalize as two fp64 operations rounded back to fp32, the table
lookup — every product and sum one separately rounded operation on numpy arrays or
scalars of the stated type; no np.percentile, no matplotlib, no torch.  The case inputs and
the loaders of tests/golden/viz/viz.npz are here too;
tests/golden/viz/make_viz_golden.py measures the restatement against numpy, matplotlib and
torch before it records the golden.
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viz", "viz.npz")
F32 = np.float32


# ---- the restatement ---------------------------------------------------------------------

def keys_of(r):
    """Order-preserving uint32 keys of an fp32 array: -0 sorts below +0."""
    b = np.ascontiguousarray(r, dtype=F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def values_of(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def lerp_coords(out, inp):
    """F.interpolate's source coordinates (align_corners=False) in fp32: i0, i1, l0, l1."""
    s = F32(inp) / F32(out)
    src = s * (np.arange(out, dtype=F32) + F32(0.5)) - F32(0.5)
    src = np.where(src < F32(0), F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int32), inp - 1)
    i1 = np.minimum(i0 + 1, inp - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def resize_np(disp, size):
    """disp (B, h, w) fp32 -> (B, H, W) fp32: hy0 * (wx0*a + wx1*b) + hy1 * (wx0*c + wx1*d)."""
    disp = np.ascontiguousarray(disp, dtype=F32)
    H, W = size
    y0, y1, hy0, hy1 = lerp_coords(H, disp.shape[1])
    x0, x1, wx0, wx1 = lerp_coords(W, disp.shape[2])
    with np.errstate(invalid="ignore"):
        top = wx0 * disp[:, y0][:, :, x0] + wx1 * disp[:, y0][:, :, x1]
        bot = wx0 * disp[:, y1][:, :, x0] + wx1 * disp[:, y1][:, :, x1]
        r = hy0[:, None] * top + hy1[:, None] * bot
    assert r.dtype == F32
    return r


def rank_of(n, percentile):
    """numpy's `linear` method on an fp32 array: (lo, hi, g, top) from the fp32 virtual index."""
    last = F32(n - 1)
    q = F32(percentile) / F32(100)
    vi = F32(last * q)
    if vi >= last:
        return n - 1, n - 1, F32(0), True
    lo = int(np.floor(vi))
    return lo, lo + 1, F32(vi - F32(lo)), False


def stats_np(r, percentile):
    """(vmin, vmax) of one resized map (H, W) fp32; NaN for both if it holds a NaN."""
    if np.isnan(r).any():
        return F32(np.nan), F32(np.nan)
    keys = np.sort(keys_of(r).ravel())
    vmin = values_of(keys[:1])[0]
    lo, hi, g, top = rank_of(keys.size, percentile)
    a0, a1 = values_of(keys[lo:lo + 1])[0], values_of(keys[hi:hi + 1])[0]
    if top:
        return vmin, a1
    with np.errstate(invalid="ignore", over="ignore"):
        d = F32(a1 - a0)
        vmax = F32(a1 - F32(d * F32(F32(1) - g))) if g >= F32(0.5) else F32(a0 + F32(d * g))
    return vmin, vmax


def index_np(r, vmin, vmax):
    """The table index of every pixel of one map (matplotlib's Normalize and Colormap.__call__)."""
    if vmin == vmax:
        t = np.zeros(r.shape, F32)
    else:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            u = (r.astype(np.float64) - np.float64(vmin)).astype(F32)
            t = (u.astype(np.float64) / (np.float64(vmax) - np.float64(vmin))).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (t * F32(256)).astype(F32)
        inside = np.where((x >= F32(0)) & (x < F32(256)), x, F32(0)).astype(np.int32)   # truncation
    return np.where(~(x >= F32(0)), 0, np.where(x >= F32(256), 255, inside)).astype(np.int32)


def colorize_np(disp, size=None, percentile=95, lut=None):
    """disp (B, 1, h, w) or (B, h, w) fp32 -> (rgb (B,H,W,3) uint8, resized (B,H,W) fp32,
    stats (B,2) fp32), the whole operator."""
    disp = np.asarray(disp, dtype=F32)
    if disp.ndim == 4:
        disp = disp[:, 0]
    size = tuple(disp.shape[1:]) if size is None else tuple(size)
    lut = load_lut() if lut is None else lut
    resized = resize_np(disp, size)
    rgb = np.zeros(resized.shape + (3,), np.uint8)
    stats = np.empty((disp.shape[0], 2), F32)
    for b, r in enumerate(resized):
        vmin, vmax = stats_np(r, percentile)
        stats[b] = vmin, vmax
        if not np.isnan(vmin):
            rgb[b] = lut[index_np(r, vmin, vmax)]
    return rgb, resized, stats


# ---- cases -------------------------------------------------------------------------------

def sigmoid_map(h, w, seed):
    """A smooth disparity-like map in (0, 1): a sigmoid of a few low-frequency waves."""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    z = 2.5 * y - 1.0
    for _ in range(4):
        fy, fx, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 2 * np.pi)
        z = z + rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fy * y + fx * x) + ph)
    return (1.0 / (1.0 + np.exp(-z))).astype(F32)


def noise_map(h, w, seed):
    return np.random.RandomState(seed).uniform(0.01, 0.99, (h, w)).astype(F32)


def build_cases():
    """name -> (disp (B,1,h,w) fp32, (H, W), percentile).  Exact-stage cases (`e_`) keep the
    size, so the resize is the identity; resize cases (`r_`) are smooth maps."""
    c = {}

    def exact(name, maps, percentile=95):
        maps = np.stack([np.asarray(m, F32) for m in maps])[:, None]
        c["e_" + name] = (maps, tuple(maps.shape[2:]), percentile)

    exact("1x1", [noise_map(1, 1, 1)])
    exact("1x7", [noise_map(1, 7, 2)])
    exact("7x3", [noise_map(7, 3, 3)])                                  # n - 1 = 20: g exactly 0
    exact("const_5x7", [np.full((5, 7), 0.37, F32)])
    exact("ties_37x50", [np.round(noise_map(37, 50, 4) / 0.02) * F32(0.02)])
    exact("16x32", [sigmoid_map(16, 32, 5)])
    exact("47x155", [sigmoid_map(47, 155, 6) * F32(0.8) + noise_map(47, 155, 7) * F32(0.1)])
    signed = np.random.RandomState(8).normal(0.3, 1.5, (16, 32)).astype(F32)
    assert signed.min() < -1 and signed.max() > 1
    exact("signed_16x32", [signed])
    holed = noise_map(16, 32, 9)
    holed[5, 11] = np.nan
    exact("nan_16x32", [holed])
    exact("batch3_16x32", [sigmoid_map(16, 32, 10), noise_map(16, 32, 11), sigmoid_map(16, 32, 12) * F32(0.25)])
    for p in (0, 50, 100):
        exact("p%d_16x32" % p, [noise_map(16, 32, 13)], p)

    def resize(h, w, H, W, seed):
        c["r_%dx%d_%dx%d" % (h, w, H, W)] = (sigmoid_map(h, w, seed)[None, None], (H, W), 95)

    resize(16, 32, 37, 50, 20)
    resize(24, 80, 47, 155, 21)
    resize(8, 8, 3, 5, 22)
    resize(20, 30, 13, 64, 23)          # down in one axis, up in the other
    return c


# ---- loaders -----------------------------------------------------------------------------

def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def load_lut(g=None):
    g = load_golden() if g is None else g
    lut = g["lut"]
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    return lut


def case_names(g, kind=None):
    names = [str(n) for n in g["names"]]
    return [n for n in names if kind is None or n.startswith(kind + "_")]


def case(g, name):
    """The recorded case: input, size, percentile and the libraries' results."""
    out = {"disp": g["in_" + name], "size": tuple(int(v) for v in g["size_" + name]),
           "percentile": int(g["pct_" + name]), "resized": g["resized_" + name],
           "vmin": g["vmin_" + name], "vmax": g["vmax_" + name], "rgb": g["rgb_" + name]}
    if name.startswith("r_"):
        out["f64"] = g["f64_" + name]
        out["floor"] = float(g["floor_" + name])
    return out


def lut_index(rgb, lut):
    """The table index of every pixel of an image made from `lut` (its rows are distinct)."""
    packed = lut[:, 0].astype(np.int64) << 16 | lut[:, 1].astype(np.int64) << 8 | lut[:, 2].astype(np.int64)
    order = np.argsort(packed)
    px = rgb[..., 0].astype(np.int64) << 16 | rgb[..., 1].astype(np.int64) << 8 | rgb[..., 2].astype(np.int64)
    pos = np.searchsorted(packed[order], px)
    pos = np.minimum(pos, 255)
    assert np.array_equal(packed[order][pos], px), "a pixel is not a table entry"
    return order[pos]
