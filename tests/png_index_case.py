"""The segment rule of the PNG index (include/md2hot.h, csrc/png.hip) restated in pure Python:
a serial inflate on png_case's bit reader and canonical tables that walks a deflate stream as
the device does, cuts the output into segments at boundary candidates and says how much of it
depends on bytes of an earlier segment; the index's byte layout; hand-made token streams whose
matches cross segment boundaries in every way the decoder has to get right.  No tests in here."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

import kitti_tree as KT
import png_case as pc

HEADER_BYTES, ENTRY_BYTES = 16, 24
MAX_SYMBOL = 258
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Walk:
    """entries: [(header_bit, symbol_bit, out_pos)] per segment; out: the inflated bytes;
    crossing: output bytes whose source chain leaves their segment; depth: the most segment
    boundaries a byte's source chain crosses."""

    def __init__(self, entries, out, crossing, depth):
        self.entries, self.out, self.crossing, self.depth = entries, out, crossing, depth


def _symbol(bits, table):
    code, length = 0, 0
    while (length, code) not in table:
        code = code << 1 | bits.take(1)
        length += 1
        assert length <= 15, "no code"
    return table[(length, code)]


def walk(deflate, total, segment_bytes):
    """The walk of a raw deflate stream (trailer bytes behind it do not matter) whose output
    is `total` bytes long, cut for segment_bytes.  A boundary candidate is a block header, the
    start of a literal/length symbol, and every byte of a stored block; a new segment starts
    at the first candidate at which the current one has produced at least segment_bytes."""
    b = pc._Bits(deflate)
    out = bytearray()
    hops = []                      # per output byte: segment boundaries its source chain crosses
    entries = [(0, 0, 0)]
    start = 0                      # where the current segment starts

    def candidate(header_bit, symbol_bit):
        nonlocal start
        if len(out) - start >= segment_bytes:
            entries.append((header_bit, symbol_bit, len(out)))
            start = len(out)

    while len(out) < total:
        header = b.pos
        candidate(header, header)
        final, kind = b.take(1), b.take(2)
        assert kind != 3
        if kind == 0:
            b.pos = (b.pos + 7) // 8 * 8
            n, nn = b.take(16), b.take(16)
            assert n ^ 0xFFFF == nn
            for _ in range(n):
                if len(out) >= total:
                    break
                candidate(header, b.pos)
                out.append(deflate[b.pos >> 3])
                hops.append(0)
                b.pos += 8
        else:
            if kind == 1:
                lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
            else:
                nlen, ndist, ncode = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for i in range(ncode):
                    cl[pc.CL_ORDER[i]] = b.take(3)
                table = pc._canonical(cl)
                lens = []
                while len(lens) < nlen + ndist:
                    s = _symbol(b, table)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.take(2))
                    elif s == 17:
                        lens += [0] * (3 + b.take(3))
                    else:
                        lens += [0] * (11 + b.take(7))
                assert len(lens) == nlen + ndist
                lit_lens, dist_lens = lens[:nlen], lens[nlen:]
            lit, dist = pc._canonical(lit_lens), pc._canonical(dist_lens)
            while len(out) < total:
                candidate(header, b.pos)
                s = _symbol(b, lit)
                if s < 256:
                    out.append(s)
                    hops.append(0)
                elif s == 256:
                    break
                else:
                    s -= 257
                    length = pc.LEN_BASE[s] + b.take(pc.LEN_EXTRA[s])
                    d = _symbol(b, dist)
                    distance = pc.DIST_BASE[d] + b.take(pc.DIST_EXTRA[d])
                    assert distance <= len(out)
                    for _ in range(min(length, total - len(out))):
                        q = len(out) - distance
                        out.append(out[q])
                        hops.append(hops[q] + (1 if q < start else 0))
        if final:
            break
    assert len(out) == total, (len(out), total)
    return Walk(entries, bytes(out), sum(1 for x in hops if x), max(hops) if hops else 0)


def capacity(h, w, segment_bytes):
    return h * (1 + 3 * w) // segment_bytes + 1


def index_nbytes(h, w, segment_bytes):
    return (HEADER_BYTES + ENTRY_BYTES * capacity(h, w, segment_bytes) + 15) // 16 * 16


def index_bytes(entries, h, w, segment_bytes):
    """The index of include/md2hot.h: u32 count, u32 segment_bytes, 8 zero bytes, the entries
    (u64 header_bit, u64 symbol_bit, u32 out_pos, u32 0), zeros to index_nbytes."""
    assert len(entries) <= capacity(h, w, segment_bytes)
    body = struct.pack("<IIQ", len(entries), segment_bytes, 0)
    body += b"".join(struct.pack("<QQII", hb, sb, op, 0) for hb, sb, op in entries)
    return np.frombuffer(body + b"\0" * (index_nbytes(h, w, segment_bytes) - len(body)), np.uint8).copy()


def read_index(index):
    """(count, segment_bytes, [(header_bit, symbol_bit, out_pos)] of the first count entries)."""
    raw = bytes(index)
    count, sb = struct.unpack_from("<II", raw, 0)
    return count, sb, [struct.unpack_from("<QQI", raw, HEADER_BYTES + ENTRY_BYTES * i) for i in range(count)]


def write_entry(index, i, header_bit=None, symbol_bit=None, out_pos=None):
    """A copy of `index` with fields of entry i replaced."""
    out = np.array(index, dtype=np.uint8, copy=True)
    hb, sb, op = struct.unpack_from("<QQI", bytes(out), HEADER_BYTES + ENTRY_BYTES * i)
    new = struct.pack("<QQII", hb if header_bit is None else header_bit, sb if symbol_bit is None else symbol_bit,
                      op if out_pos is None else out_pos, 0)
    out[HEADER_BYTES + ENTRY_BYTES * i:HEADER_BYTES + ENTRY_BYTES * (i + 1)] = np.frombuffer(new, np.uint8)
    return out


def index_of(stream, segment_bytes):
    """(index bytes, Walk) of a png_ops.PngStream by the restatement."""
    total = stream.height * (1 + 3 * stream.width)
    w = walk(stream.data[:-4], total, segment_bytes)
    return index_bytes(w.entries, stream.height, stream.width, segment_bytes), w


# ------------------------------------------------------------------ streams of the libraries
H, W, S = 24, 100, 1024          # 7224 scanline bytes: 7 segments of 1024..1281
ROW = 1 + 3 * W
TOTAL = H * ROW


def _scene(rng, h, w):
    """A frame with smooth parts, repeats and noise: literals and matches near and far."""
    img = KT.image(rng, h, w)
    if h >= 8 and w >= 16:
        img[h // 2:, :w // 2] = img[:h - h // 2, w - w // 2:]          # a far repeat
        img[: h // 4] = (np.arange(w)[None, :, None] * 3) & 255         # rows Sub and Up flatten
    return img


def _pillow(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG", **kw)
    return buf.getvalue()


ZLIB_MODES = {
    "default": dict(),
    "filtered": dict(strategy=zlib.Z_FILTERED),
    "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": dict(strategy=zlib.Z_RLE),
    "fixed": dict(strategy=zlib.Z_FIXED),
    "sync_flush": dict(flush_every=512, flush_mode=zlib.Z_SYNC_FLUSH),       # an empty stored block on
    "full_flush": dict(flush_every=1024, flush_mode=zlib.Z_FULL_FLUSH),      # every boundary of S = 1024
    "sync_flush_near": dict(flush_every=1023, flush_mode=zlib.Z_SYNC_FLUSH),
    "level0_flush": dict(level=0, flush_every=512, flush_mode=zlib.Z_SYNC_FLUSH),   # ... behind a stored block
    "level0_flush_near": dict(level=0, flush_every=700, flush_mode=zlib.Z_SYNC_FLUSH),
}


def library_cases(seed=3):
    """{name: png bytes}: Pillow's saves and zlib's strategies and flushes on a 24 x 100 frame
    (7 segments at S = 1024), and the 1 x 1 and 1 x 8192 frames."""
    rng = np.random.default_rng(seed)
    img = _scene(rng, H, W)
    filters = rng.integers(0, 5, H).tolist()
    cases = {"pillow_%d" % level: _pillow(img, compress_level=level) for level in (0, 1, 6, 9)}
    cases["pillow_optimize"] = _pillow(img, optimize=True)
    for name, kw in ZLIB_MODES.items():
        cases["zlib_" + name] = pc.write_png(img, filters, **kw)
    cases["1x1"] = pc.write_png(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), [pc.SUB])
    cases["1x8192"] = pc.write_png(_scene(rng, 1, 8192), [pc.PAETH], level=6)
    return cases


MIXED_SIZES = [(24, 100), (1, 1), (7, 5), (66, 67), (3, 700), (40, 33), (130, 8), (24, 100), (9, 341)]


def mixed_batch(seed=4):
    """PNG files of MIXED_SIZES: frames of one segment next to frames of three and more
    (none of exactly two: every multi-segment case has at least 3); Pillow's and zlib's streams."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(MIXED_SIZES):
        img = _scene(rng, h, w)
        out.append(_pillow(img, compress_level=(1, 6, 9)[i % 3]) if i % 2 else
                   pc.write_png(img, rng.integers(0, 5, h).tolist(), level=(0, 6, 9)[i % 3]))
    return out


# ------------------------------------------------------------------ hand-made token streams


def _literals(rng, n):
    return [int(x) for x in rng.integers(5, 256, n)]


def _finish(tokens, rng):
    """Pads with literals to TOTAL bytes and settles the filter bytes."""
    have = len(pc.expand(tokens))
    assert have <= TOTAL, have
    tokens = tokens + _literals(rng, TOTAL - have)
    return pc.settle_filter_bytes(tokens, ROW, rng)


def _png(deflate, raw):
    assert len(raw) == TOTAL
    return pc.png_bytes(H, W, pc.zlib_wrap(deflate, raw))


def _fixed(tokens):
    bw = pc.BitWriter()
    bw.fixed_block(tokens)
    return _png(bw.bytes(), pc.expand(tokens))


def dynamic_code():
    """(lit_lens, dist_lens, length_ops) of a complete dynamic code over all 286 literal/length
    and all 30 distance symbols: literals at 9 bits but the first 16 at 8 (272/512), the end
    and the 29 length symbols at 6 (240/512): 512/512; the first 2 distance symbols at 4 bits,
    the other 28 at 5 (2/16 + 28/32 = 1)."""
    lit = [8] * 16 + [9] * 240 + [6] * 30
    dist = [4] * 2 + [5] * 28
    return lit, dist, list(lit + dist)


def _dynamic(tokens):
    lit, dist, ops = dynamic_code()
    bw = pc.BitWriter()
    bw.dynamic_block(tokens, lit, dist, ops)
    return _png(bw.bytes(), pc.expand(tokens))


def handmade_cases(seed=11):
    """{name: png bytes} of 24 x 100 frames (7 segments at S = 1024) whose matches cross the
    boundaries: see the test of each name in test_png_index_gpu.py."""
    rng = np.random.default_rng(seed)
    cases = {}

    # a match whose source starts in one segment and ends in the next (a boundary lies between
    # two symbols, so the match itself is never cut): at 1100, 200 bytes from 950..1149, the
    # boundary at 1024; then one that ends exactly where the next boundary would be looked for
    t = _literals(rng, 1100) + [(200, 150)] + _literals(rng, 600) + [(258, 1000)]
    cases["match_across_boundary"] = _fixed(_finish(t, rng))

    # a period copy whose source starts before the boundary: the boundary falls at 1024 (all
    # literals before it), the match at 1026 repeats 5 bytes of which 3 lie before 1024
    t = _literals(rng, 1026) + [(200, 5)]
    cases["period_from_before_boundary"] = _fixed(_finish(t, rng))

    # segment 3 copies bytes that segment 2 copied from segment 1
    t = _literals(rng, 1100) + [(100, 1000)] + _literals(rng, 2200 - 1200) + [(100, 1100)]
    t += _literals(rng, 3300 - 2300) + [(100, 1100)]
    cases["chain_through_segments"] = _fixed(_finish(t, rng))

    # one dynamic block spanning the whole image: every entry but the first is mid-block
    t = _literals(rng, 1500) + [(258, 1400)] + _literals(rng, 1500) + [(30, 3000), (3, 1), (258, 2)]
    cases["one_dynamic_block"] = _dynamic(_finish(t, rng))

    # one fixed block likewise
    cases["one_fixed_block"] = _fixed(_finish(list(t), rng))

    # a stored block cut by a boundary (and by two more), then a fixed block reaching back into it
    raw_tokens = _finish(_literals(rng, 3000) + [(258, 2500)] * 3, rng)
    raw = pc.expand(raw_tokens)
    bw = pc.BitWriter()
    bw.stored_block(raw[:3000], final=False)
    bw.fixed_block(raw_tokens[3000:])
    cases["stored_block_cut"] = _png(bw.bytes(), raw)
    return cases


def far_case(seed=12):
    """A 5 x 2400 frame (36005 scanline bytes) with a match at distance 32768 measured from
    the first byte of a segment: all literals (boundaries at multiples of 1024) up to 33792 =
    33 * 1024, then a match of 100 bytes from 1024."""
    rng = np.random.default_rng(seed)
    h, w = 5, 2400
    total = h * (1 + 3 * w)
    t = _literals(rng, 33 * 1024) + [(100, 32768)]
    t += _literals(rng, total - len(pc.expand(t)))
    pc.settle_filter_bytes(t, 1 + 3 * w, rng)
    bw = pc.BitWriter()
    bw.fixed_block(t)
    raw = pc.expand(t)
    return pc.png_bytes(h, w, pc.zlib_wrap(bw.bytes(), raw))
