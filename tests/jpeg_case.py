"""Shared cases of the JPEG decoder tests and a plain numpy restatement of the decoder.

The cases are written by Pillow in memory from seeded arrays.  The restatement is the
sequential decoder in the written rules of the decoder: canonical Huffman
codes, DC prediction, dequantisation, the accurate-integer inverse DCT (columns with a
rounding shift of 11, rows with 18, constants at 13 bits), component planes cropped before
upsampling, libjpeg's triangle / 3:1 chroma filters with replication on planes at most two
samples wide, and the 16-bit fixed-point colour conversion.  `fixed_point_slots` restates
the parallel synchronisation of the entropy decoder: subsequences of SUB_BITS bits whose
entry states are iterated until nothing changes.
"""
import io

import numpy as np
from PIL import Image

from monodepth2_amd.jpeg_ops import ZIGZAG, parse_jpeg

SUB_BITS = 1024
SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


# ------------------------------------------------------------------ cases
def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def textured(h, w, seed):
    """A gradient with a little structure and noise: what a photograph costs to code."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([96 + 0.11 * x + 40 * np.sin(y / 7.0), 128 + 50 * np.cos(x / 13.0 + y / 29.0),
                     200 - 0.3 * y - 0.05 * x], -1)
    return np.clip(base + rs.normal(0, 9, (h, w, 3)), 0, 255).astype(np.uint8)


def flat(h, w, seed):
    return np.full((h, w, 3), (seed * 37 % 256, 90, 200), np.uint8)


def encode(arr, sampling="4:2:0", quality=92, optimize=False, **extra) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[sampling], optimize=optimize,
                              **extra)
    return buf.getvalue()


def build_cases():
    """name -> JPEG file bytes.  Small first; the names say what each is there for."""
    cases = {}
    seed = 0

    def add(name, make, h, w, **kw):
        nonlocal seed
        seed += 1
        cases[name] = encode(make(h, w, seed), **kw)

    for samp in SUBSAMPLING:
        tag = samp.replace(":", "")
        for h, w in ((1, 1), (8, 8), (16, 16), (17, 33), (37, 53)):   # smallest, exact MCUs, partial MCUs
            add(f"size_{h}x{w}_{tag}", textured, h, w, sampling=samp)
    for samp in ("4:2:2", "4:2:0"):
        tag = samp.replace(":", "")
        for w in (3, 4):                                              # the replication rule
            add(f"narrow_9x{w}_{tag}", noise, 9, w, sampling=samp)
        for w in (5, 6):                                              # the narrowest fancy filter
            add(f"narrow_9x{w}_{tag}", noise, 9, w, sampling=samp)
    for h in (1, 2, 3):                                               # row replication
        add(f"low_{h}x21_420", noise, h, 21, sampling="4:2:0")
    add("flat_16x16_420", flat, 16, 16, sampling="4:2:0")            # shorter than one subsequence
    add("noise_64x96_q100_444", noise, 64, 96, sampling="4:4:4", quality=100)        # slow synchronisation
    add("noise_192x320_q100_444", noise, 192, 320, sampling="4:4:4", quality=100)    # more subsequences than threads
    add("kitti_375x1242_q92_422", textured, 375, 1242, sampling="4:2:2", quality=92)
    for samp in SUBSAMPLING:
        tag = samp.replace(":", "")
        for q in (30, 92, 100):
            for opt in (False, True):
                add(f"mix_24x40_{tag}_q{q}{'_opt' if opt else ''}", textured, 24, 40, sampling=samp, quality=q,
                    optimize=opt)
    return cases


_CASES = None


def cases():
    """The case files, built once per process."""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


_PILLOW = {}


def pillow_rgb(name) -> np.ndarray:
    """The reference, computed once per case and never changed."""
    if name not in _PILLOW:
        a = np.asarray(Image.open(io.BytesIO(cases()[name])).convert("RGB"))
        a.setflags(write=False)
        _PILLOW[name] = a
    return _PILLOW[name]


def cut_in_half(data: bytes) -> bytes:
    """The file with the second half of its entropy-coded segment removed and the EOI put
    back: parses as supported, decodes short."""
    sos = data.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    assert data[-2:] == b"\xff\xd9"
    body = data[start:-2]
    half = body[:len(body) // 2]
    if half.endswith(b"\xff"):      # never leave half a stuffed pair
        half = half[:-1]
    return data[:start] + half + b"\xff\xd9"


# ------------------------------------------------------------------ entropy decoding
class Huffman:
    """Canonical codes of one DHT table: a 16-bit lookup of (length, symbol)."""

    def __init__(self, counts, values):
        self.length = np.zeros(1 << 16, np.uint8)
        self.symbol = np.zeros(1 << 16, np.uint8)
        code, k = 0, 0
        for l in range(1, 17):
            for _ in range(counts[l - 1]):
                lo = code << (16 - l)
                self.length[lo:lo + (1 << (16 - l))] = l
                self.symbol[lo:lo + (1 << (16 - l))] = values[k]
                code += 1
                k += 1
            code <<= 1
        self.length = self.length.tolist()
        self.symbol = self.symbol.tolist()


class Entropy:
    """The entropy-coded segment of a parsed stream and the geometry of its scan."""

    def __init__(self, s):
        self.s = s
        self.hs, self.vs = s.factors[0]
        self.mcux = -(-s.width // (8 * self.hs))
        self.mcuy = -(-s.height // (8 * self.vs))
        self.bpm = self.hs * self.vs + 2
        self.total_blocks = self.mcux * self.mcuy * self.bpm
        self.total_bits = 8 * len(s.data)
        self.padded = s.data + b"\0" * 8   # zeros past the end
        self.tabs = [(Huffman(*s.huff[(0, s.dc[c])]), Huffman(*s.huff[(1, s.ac[c])])) for c in range(3)]
        self.nsub = max(-(-self.total_bits // SUB_BITS), 1)

    def comp(self, b):
        ny = self.hs * self.vs
        return (0, b) if b < ny else (b - ny + 1, 0)

    def peek(self, p):
        i = p >> 3
        return (int.from_bytes(self.padded[i:i + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF

    def decode(self, state, end, sink=None, g0=0, boundaries=None):
        """From `state` = (bit, block in MCU, zigzag index) until the bit position reaches
        `end`: (exit state, blocks completed).  sink(g, k, value) receives the coefficients
        (DC as a difference) of block g0 + n; with a sink nothing at or past the image's
        block count is decoded.  boundaries: list filled with the state at the first symbol
        at or after every multiple of SUB_BITS (the sequential decoder's slots)."""
        p, b, k = state
        end = min(end, self.total_bits)
        done = 0
        c = self.comp(b)[0]
        while p < end:
            if sink is not None and g0 + done >= self.total_blocks:
                break
            if boundaries is not None:
                while len(boundaries) * SUB_BITS <= p:
                    boundaries.append((p, b, k))
            H = self.tabs[c][1 if k else 0]
            look = self.peek(p)
            code16 = look >> 16
            ln = H.length[code16]
            sym = H.symbol[code16] if ln else 0
            ln = ln or 16
            n = (sym & 15) if k else min(sym, 15)
            if p + ln + n > self.total_bits:
                p = self.total_bits
                break
            v = 0
            if n:
                raw = ((look << ln) & 0xFFFFFFFF) >> (32 - n)
                v = raw - (1 << n) + 1 if raw < (1 << (n - 1)) else raw
            p += ln + n
            block_done = False
            if k == 0:
                if sink is not None:
                    sink(g0 + done, 0, v)
                k = 1
            else:
                r = sym >> 4
                if n == 0:
                    if r == 15:
                        k += 16
                    else:
                        block_done = True
                else:
                    k += r
                    if k <= 63:
                        if sink is not None:
                            sink(g0 + done, k, v)
                        k += 1
                if k > 63:
                    block_done = True
            if block_done:
                done += 1
                k = 0
                b = (b + 1) % self.bpm
                c = self.comp(b)[0]
        return (p, b, k), done


def sequential_coefficients(s):
    """The sequential decode: per component an int32 array (blocks down, blocks across, 64)
    of coefficients in natural order with the DC prediction applied, the number of blocks
    decoded, and the slot states at the subsequence boundaries."""
    E = Entropy(s)
    dims = [(E.mcuy * (E.vs if c == 0 else 1), E.mcux * (E.hs if c == 0 else 1)) for c in range(3)]
    coef = [np.zeros(d + (64,), np.int32) for d in dims]
    pred = [0, 0, 0]

    def sink(g, k, v):
        m, b = divmod(g, E.bpm)
        c, jc = E.comp(b)
        hs, vs = (E.hs, E.vs) if c == 0 else (1, 1)
        my, mx = divmod(m, E.mcux)
        by, bx = my * vs + jc // hs, mx * hs + jc % hs
        if k == 0:
            pred[c] += v
            v = pred[c]
        coef[c][by, bx, ZIGZAG[k]] = v

    boundaries = []
    state, done = E.decode((0, 0, 0), E.total_bits, sink, 0, boundaries)
    while len(boundaries) < E.nsub:
        boundaries.append(state)   # no symbol starts at or after these boundaries
    return coef, done, boundaries, E


def fixed_point_slots(s):
    """The synchronisation restated: slot 0 true, slot i the guess (SUB_BITS * i, 0, 0); every
    subsequence whose entry slot changed in the last round is decoded again from it and its
    exit written to the next slot; stop when nothing changes.  Returns (slots, blocks per
    subsequence, rounds, subsequence decodes)."""
    E = Entropy(s)
    slots = [(SUB_BITS * i, 0, 0) for i in range(E.nsub + 1)]
    counts = [0] * E.nsub
    dirty = set(range(E.nsub))
    rounds = decodes = 0
    while dirty:
        rounds += 1
        nxt = set()
        updates = []
        for i in sorted(dirty):
            st, counts[i] = E.decode(slots[i], SUB_BITS * (i + 1))
            decodes += 1
            if st != slots[i + 1]:
                updates.append((i + 1, st))
        for i, st in updates:     # all of a round's decodes read the slots of the round before
            slots[i] = st
            if i < E.nsub:
                nxt.add(i)
        dirty = nxt
    return slots, counts, rounds, decodes, E


# ------------------------------------------------------------------ pixels
C = dict(c298=2446, c390=3196, c541=4433, c765=6270, c899=7373, c1175=9633, c1501=12299, c1847=15137,
         c1961=16069, c2053=16819, c2562=20995, c3072=25172)


def idct8(v, shift):
    """The eight-point transform along the last axis of an int64 array, descaled by `shift`."""
    i0, i1, i2, i3, i4, i5, i6, i7 = [v[..., j] for j in range(8)]
    z1 = (i2 + i6) * C["c541"]
    tmp2 = z1 - i6 * C["c1847"]
    tmp3 = z1 + i2 * C["c765"]
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C["c1175"]
    t0, t1, t2, t3 = t0 * C["c298"], t1 * C["c2053"], t2 * C["c3072"], t3 * C["c1501"]
    z1, z2 = -z1 * C["c899"], -z2 * C["c2562"]
    z3, z4 = -z3 * C["c1961"] + z5, -z4 * C["c390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    half = 1 << (shift - 1)
    out = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    return np.stack([(o + half) >> shift for o in out], -1)


def samples(coef, quant):
    """(blocks down, blocks across, 64) coefficients -> the uint8 sample plane."""
    hb, wb, _ = coef.shape
    x = (coef.astype(np.int64) * np.asarray(quant, np.int64)).reshape(hb, wb, 8, 8)
    x = idct8(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)   # columns
    x = idct8(x, 18)                                      # rows
    x = np.clip(x + 128, 0, 255).astype(np.uint8)
    return x.transpose(0, 2, 1, 3).reshape(hb * 8, wb * 8)


def upsample_h(c, mode):
    """One plane doubled across: mode "triangle" on samples, or "v" on the 3:1 row sums."""
    c = c.astype(np.int64)
    n = c.shape[1]
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    if mode == "triangle":
        even, odd = (3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2
        even[:, 0], odd[:, -1] = c[:, 0], c[:, -1]
    else:
        even, odd = (3 * c + left + 8) >> 4, (3 * c + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * c[:, 0] + 8) >> 4, (4 * c[:, -1] + 7) >> 4
    out = np.empty((c.shape[0], 2 * n), np.int64)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out


def upsample(plane, h, w, hs, vs):
    """A chroma sample plane -> (h, w) at full resolution."""
    cw, ch = -(-w // hs), -(-h // vs)
    c = plane[:ch, :cw]                       # cropped before anything looks at its edges
    if hs == 1:
        return c.astype(np.int64)
    if cw <= 2:                               # libjpeg's plain replication, both ways
        return np.repeat(np.repeat(c, vs, 0), 2, 1)[:h, :w].astype(np.int64)
    if vs == 1:
        return upsample_h(c, "triangle")[:, :w]
    c = c.astype(np.int64)
    above = np.concatenate([c[:1], c[:-1]], 0)
    below = np.concatenate([c[1:], c[-1:]], 0)
    rows = np.empty((2 * ch, cw), np.int64)
    rows[0::2], rows[1::2] = 3 * c + above, 3 * c + below
    return upsample_h(rows, "v")[:h, :w]


def decode_np(s) -> np.ndarray:
    """The whole sequential decoder: a parsed stream -> (h, w, 3) uint8 RGB."""
    coef, done, _, E = sequential_coefficients(s)
    assert done == E.total_blocks, (done, E.total_blocks)
    planes = [samples(coef[c], s.quant[c]) for c in range(3)]
    h, w = s.height, s.width
    Y = planes[0][:h, :w].astype(np.int64)
    cb = upsample(planes[1], h, w, E.hs, E.vs) - 128
    cr = upsample(planes[2], h, w, E.hs, E.vs) - 128
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def parsed(name):
    s = parse_jpeg(cases()[name])
    assert s is not None, name
    return s
