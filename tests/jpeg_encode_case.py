"""Shared cases of the JPEG encoder tests and a plain numpy restatement of the encoder.

The restatement follows the written rules of the encoder: 16-bit fixed-point
RGB -> YCbCr, edge extension (last pixel across before downsampling; down, the rows up to a
multiple of the vertical factor, then the downsampled last row), box downsampling with the
alternating bias, the accurate integer forward DCT (rows then columns, constants at 13 bits),
quantisation by 8 q with rounding half away from zero, one interleaved scan with dummy
blocks, and the standard Huffman tables.  Its output is the unstuffed entropy-coded segment.
The reference of every test is Pillow's file, made once per case and never changed.
"""
import io

import numpy as np
from PIL import Image

from jpeg_case import C, SUBSAMPLING, flat, noise, textured
from monodepth2_amd.jpeg_ops import STD_HUFF, ZIGZAG, quality_tables, sampling_class, standard_stream

FACTORS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
QUALITIES = (30, 75, 92, 100)
SIZES = ((1, 1), (8, 8), (16, 16), (9, 3), (17, 33), (37, 53), (24, 40), (23, 15), (7, 250))
MAKERS = {"textured": textured, "noise": noise, "flat": flat}


def build_cases():
    """name -> (maker, h, w, seed, sampling, quality).  Small first; the grid of the issue,
    then the cases that are there for one property each."""
    cases = {}
    seed = 100
    for samp in SUBSAMPLING:
        tag = samp.replace(":", "")
        for q in QUALITIES:
            for h, w in SIZES:
                seed += 1
                cases[f"grid_{h}x{w}_{tag}_q{q}"] = ("textured", h, w, seed, samp, q)
    cases["flat_16x16_420_q75"] = ("flat", 16, 16, 7, "4:2:0", 75)            # six blocks in two words
    cases["noise_64x96_444_q100"] = ("noise", 64, 96, 8, "4:4:4", 100)         # long codes, FF bytes
    cases["textured_64x96_420_q30"] = ("textured", 64, 96, 9, "4:2:0", 30)     # runs of 16 zeros
    cases["kitti_375x1242_420_q92"] = ("textured", 375, 1242, 10, "4:2:0", 92)
    return cases


CASES = build_cases()
MIXED = ("grid_37x53_444_q92", "grid_17x33_422_q30", "grid_24x40_420_q75", "grid_7x250_420_q100",
         "noise_64x96_444_q100", "grid_1x1_422_q75", "flat_16x16_420_q75", "grid_23x15_444_q30")

_FRAMES, _PILLOW = {}, {}


def frame(name) -> np.ndarray:
    if name not in _FRAMES:
        maker, h, w, seed, _, _ = CASES[name]
        a = MAKERS[maker](h, w, seed)
        a.setflags(write=False)
        _FRAMES[name] = a
    return _FRAMES[name]


def pillow_file(name) -> bytes:
    """The reference, computed once per case and never changed."""
    if name not in _PILLOW:
        _, _, _, _, samp, q = CASES[name]
        buf = io.BytesIO()
        Image.fromarray(frame(name)).save(buf, "JPEG", quality=q, subsampling=SUBSAMPLING[samp])
        _PILLOW[name] = buf.getvalue()
    return _PILLOW[name]


# ------------------------------------------------------------------ samples
def ycc(rgb):
    """Rule 1: (h, w, 3) uint8 -> Y, Cb, Cr int64 planes."""
    r, g, b = [rgb[..., i].astype(np.int64) for i in range(3)]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def component_plane(full, hs, vs):
    """Rules 2 and 3: a full-resolution plane -> the component's samples on its own block
    grid, downsampled by hs x vs with clamped reads."""
    h, w = full.shape
    cw, ch = -(-w // hs), -(-h // vs)
    wb, hb = -(-cw // 8), -(-ch // 8)
    cy = np.minimum(np.arange(hb * 8), ch - 1)      # the downsampled last row is repeated
    cx = np.arange(wb * 8)
    acc = np.zeros((hb * 8, wb * 8), np.int64)
    for dy in range(vs):
        rows = np.minimum(cy * vs + dy, h - 1)      # rows extended to a multiple of vs
        for dx in range(hs):
            cols = np.minimum(cx * hs + dx, w - 1)  # the last pixel repeated before downsampling
            acc += full[rows][:, cols]
    if hs * vs == 1:
        return acc
    bias = (cx & 1) if vs == 1 else 1 + (cx & 1)
    return (acc + bias[None, :]) >> (1 if vs == 1 else 2)


# ------------------------------------------------------------------ transform
def fdct8(d, first):
    """Rule 4: the eight-point forward transform along the last axis.  first: the row pass
    (outputs 0 and 4 scaled up by 2 bits, the others descaled by 11); else the column pass
    (2 and 15)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., j] for j in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d0 + d7, d0 - d7, d1 + d6, d1 - d6
    tmp2, tmp5, tmp3, tmp4 = d2 + d5, d2 - d5, d3 + d4, d3 - d4
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    n = 11 if first else 15
    if first:
        o0, o4 = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        o0, o4 = descale(tmp10 + tmp11, 2), descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * C["c541"]
    o2 = descale(z1 + tmp13 * C["c765"], n)
    o6 = descale(z1 - tmp12 * C["c1847"], n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * C["c1175"]
    t4, t5, t6, t7 = tmp4 * C["c298"], tmp5 * C["c2053"], tmp6 * C["c3072"], tmp7 * C["c1501"]
    z1, z2 = -z1 * C["c899"], -z2 * C["c2562"]
    z3, z4 = -z3 * C["c1961"] + z5, -z4 * C["c390"] + z5
    o7, o5, o3, o1 = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], -1)


def quantised(plane, quant):
    """Rules 4 and 5: a sample plane on its block grid -> (blocks down, blocks across, 64)
    quantised coefficients in natural order."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    x = (plane - 128).reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3)
    x = fdct8(x, True)                                     # rows
    x = fdct8(x.swapaxes(-1, -2), False).swapaxes(-1, -2)  # columns
    q8 = 8 * np.asarray(quant, np.int64).reshape(8, 8)
    mag = (np.abs(x) + (q8 >> 1)) // q8
    return (np.sign(x) * mag).reshape(hb, wb, 64)


# ------------------------------------------------------------------ codes
def huffman_codes(counts, values):
    """symbol -> (code, length) of a DHT table (canonical codes)."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def value(self, v, size):
        """Rule 7: a value of category `size`; negative ones as v - 1 in `size` bits."""
        if size:
            self.put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)

    def finish(self) -> bytes:
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)          # the last byte is filled with 1-bits
        return self.acc.to_bytes(self.n // 8, "big")


def encode_np(rgb, sampling="4:2:0", quality=92):
    """The whole sequential encoder: (h, w, 3) uint8 -> a JpegStream whose data is the
    unstuffed entropy-coded segment."""
    hs, vs = FACTORS[sampling]
    h, w, _ = rgb.shape
    luma_q, chroma_q = quality_tables(quality)
    y, cb, cr = ycc(rgb)
    coef = [quantised(component_plane(y, 1, 1), luma_q), quantised(component_plane(cb, hs, vs), chroma_q),
            quantised(component_plane(cr, hs, vs), chroma_q)]
    zz = np.asarray(ZIGZAG)
    coef = [c[..., zz].tolist() for c in coef]
    hb0, wb0 = len(coef[0]), len(coef[0][0])
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    dc_codes = [huffman_codes(*STD_HUFF[(0, t)]) for t in (0, 1)]
    ac_codes = [huffman_codes(*STD_HUFF[(1, t)]) for t in (0, 1)]
    out = BitWriter()
    pred = [0, 0, 0]
    zero = [0] * 64
    for my in range(mcuy):
        for mx in range(mcux):
            blocks = []
            for jy in range(vs):
                for jx in range(hs):
                    by, bx = my * vs + jy, mx * hs + jx
                    if by < hb0 and bx < wb0:
                        blocks.append((0, coef[0][by][bx]))
                    else:                       # rule 6: a dummy block repeats the DC before it
                        blocks.append((0, [blocks[-1][1][0]] + zero[1:]))
            blocks.append((1, coef[1][my][mx]))
            blocks.append((2, coef[2][my][mx]))
            for c, blk in blocks:
                t = 0 if c == 0 else 1
                diff = blk[0] - pred[c]
                pred[c] = blk[0]
                size = abs(diff).bit_length()
                out.put(*dc_codes[t][size])
                out.value(diff, size)
                run = 0
                for k in range(1, 64):
                    v = blk[k]
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        out.put(*ac_codes[t][0xF0])
                        run -= 16
                    size = abs(v).bit_length()
                    out.put(*ac_codes[t][run << 4 | size])
                    out.value(v, size)
                    run = 0
                if run:
                    out.put(*ac_codes[t][0x00])
    return standard_stream(h, w, sampling_class(sampling), quality, out.finish())
