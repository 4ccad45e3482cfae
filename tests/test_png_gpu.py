"""png_ops.decode_png_batch (csrc/png.hip) against Pillow, byte for byte: the five filters on
every row position, zlib's block kinds, strategies and flushes, deflate blocks written by hand
(the longest distance, short periods, the extra-bit edges of the length codes, a match that
ends the image, bytes behind a complete image), dynamic blocks at their edges (tiny
alphabets, a single distance code, a repeat across the literal/length | distance boundary),
damaged streams in the middle of a batch (exactly their status bit, neighbours untouched) and
one full-size frame.  Every frame sits between guard bytes that must stay as they were."""
import io
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import kitti_tree as KT
import png_case as pc

pytestmark = pytest.mark.gpu

GUARD = 64
ST_BLOCK, ST_CODE, ST_END, ST_DIST, ST_FILTER, ST_ADLER = 1, 2, 4, 8, 16, 32


def pillow(png):
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))


def layout(streams):
    """Frame offsets (multiples of 16) with at least GUARD bytes before, between and behind."""
    offsets, pos = [], GUARD
    for s in streams:
        offsets.append(pos)
        pos = (pos + s.height * s.width * 3 + GUARD + 15) // 16 * 16
    return offsets, pos


def decode(pngs):
    """[(frame or None where the status is not 0, status)] of a batch; checks the guards."""
    from monodepth2_amd.png_ops import decode_png_batch, parse_png
    streams = [parse_png(p) for p in pngs]
    assert all(s is not None for s in streams)
    offsets, total = layout(streams)
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    status = decode_png_batch(streams, out, offsets).cpu().tolist()
    host = out.cpu().numpy()
    frames, keep = [], np.ones(total, bool)
    for s, o, st in zip(streams, offsets, status):
        n = s.height * s.width * 3
        keep[o:o + n] = False
        frames.append(host[o:o + n].reshape(s.height, s.width, 3).copy())
    assert (host[keep] == 0xA5).all(), "a byte outside the frames was written"
    return list(zip(frames, status))


def assert_decodes(png):
    (frame, status), = decode([png])
    assert status == 0
    assert np.array_equal(frame, pillow(png))


def harsh(rng, h, w):
    """Random bytes with runs of 0 and 255 next to each other: Avg's 9-bit sums, Paeth's ties."""
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    pick = rng.integers(0, 4, (h, w, 3))
    img[pick == 0] = 0
    img[pick == 1] = 255
    return img


# ------------------------------------------------------------------ unfilter
SIZES = [(1, 1), (5, 1), (1, 7), (7, 5), (66, 67), (130, 3)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("filt", [pc.NONE, pc.SUB, pc.UP, pc.AVG, pc.PAETH, "mixed"])
def test_unfilter(size, filt):
    h, w = size
    rng = np.random.default_rng(100 * h + w)
    filters = rng.integers(0, 5, h).tolist() if filt == "mixed" else [filt] * h
    assert_decodes(pc.write_png(harsh(rng, h, w), filters))


def paeth_cases(img):
    """How often each tie of the Paeth predictor occurs in an image: (pa == pb, pb == pc, pa == pc)."""
    h, w, _ = img.shape
    flat = np.zeros((h + 1, 3 * w + 3), np.int64)
    flat[1:, 3:] = img.reshape(h, 3 * w)
    a, b, c = flat[1:, :-3], flat[:-1, 3:], flat[:-1, :-3]
    pa, pb, pc_ = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return int(((pa == pb) & (pa < pc_)).sum()), int(((pb == pc_) & (pb < pa)).sum()), int(((pa == pc_) & (pa < pb)).sum())


def test_paeth_ties():
    rng = np.random.default_rng(7)
    img = harsh(rng, 9, 11)
    # (left, above, above-left) of the pixels (1, 1), (1, 3), (1, 5): pa == pb, pb == pc, pa == pc
    for k, (a, b, c) in enumerate([(10, 10, 5), (12, 6, 10), (6, 12, 10)]):
        img[0, 2 * k], img[0, 2 * k + 1], img[1, 2 * k] = c, b, a
    assert min(paeth_cases(img)) > 0, paeth_cases(img)
    assert_decodes(pc.write_png(img, [pc.PAETH] * 9))


# ------------------------------------------------------------------ inflate, zlib's streams
ZLIB_MODES = {
    "level0": dict(level=0),
    "fixed": dict(strategy=zlib.Z_FIXED),
    "level9": dict(level=9),
    "rle": dict(strategy=zlib.Z_RLE),
    "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY),
    "sync_flush": dict(flush_every=1000, flush_mode=zlib.Z_SYNC_FLUSH),
    "full_flush": dict(flush_every=1000, flush_mode=zlib.Z_FULL_FLUSH),
}


def zlib_case(size, mode):
    h, w = size
    rng = np.random.default_rng(h)
    img = KT.image(rng, h, w)
    filters = rng.integers(0, 5, h).tolist() if h < 100 else [pc.SUB] * h
    return pc.write_png(img, filters, **ZLIB_MODES[mode])


@pytest.mark.parametrize("size", [(66, 67), (150, 150)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", list(ZLIB_MODES))
def test_zlib_streams(size, mode):
    from monodepth2_amd.png_ops import parse_png
    png = zlib_case(size, mode)
    first = pc.first_block(parse_png(png).data)
    assert first["type"] == {"level0": 0, "fixed": 1}.get(mode, 2)
    if mode == "level0" and size == (150, 150):   # two stored blocks, the first as long as one can be
        assert struct.unpack_from("<H", parse_png(png).data, 1)[0] == 65535 and not first["final"]
    assert_decodes(png)


def test_constant_image():
    png = pc.write_png(np.full((40, 50, 3), 77, np.uint8), level=9)   # length 258 at distance 1 throughout
    assert_decodes(png)


# ------------------------------------------------------------------ inflate, blocks by hand
def by_hand(h, w, tokens, seed=0, adler_of=None, junk=b""):
    """The file of a fixed-Huffman block of `tokens`, their row-start literals settled."""
    rng = np.random.default_rng(seed)
    tokens = pc.settle_filter_bytes(list(tokens), 1 + 3 * w, rng)
    raw = pc.expand(tokens)
    bw = pc.BitWriter()
    bw.fixed_block(tokens)
    return pc.png_bytes(h, w, pc.zlib_wrap(bw.bytes() + junk, raw if adler_of is None else raw[:adler_of])), raw


def literals(rng, n):
    return rng.integers(0, 256, n).tolist()


def longest_distance_case():
    rng = np.random.default_rng(1)
    h, w = 111, 100
    total = h * (1 + 3 * w)
    tokens = literals(rng, 32768) + [(258, 32768)]
    tokens += literals(rng, total - 32768 - 258)
    return by_hand(h, w, tokens, 1)


def period_case(distance):
    rng = np.random.default_rng(distance)
    h, w = 4, 90
    total = h * (1 + 3 * w)
    tokens = literals(rng, 65) + [(258, distance)] + literals(rng, 40) + [(258, distance), (258, distance)]
    tokens += literals(rng, total - 65 - 40 - 3 * 258)
    return by_hand(h, w, tokens, distance)


def lengths_case(end_with_match):
    rng = np.random.default_rng(3)
    h, w = 4, 90
    total = h * (1 + 3 * w)
    tokens = literals(rng, 70) + [(3, 5)] + literals(rng, 9) + [(10, 7), (11, 64)] + literals(rng, 5) + [(257, 70)]
    tokens += [(258, 1), (4, 2), (12, 300)]
    done = len(pc.expand(tokens))
    tokens += literals(rng, total - done - 20) + ([(20, 9)] if end_with_match else literals(rng, 20))
    return by_hand(h, w, tokens, 3)


def test_longest_distance():
    png, raw = longest_distance_case()
    assert len(raw) == 111 * 301 and raw[32768:32768 + 258] == raw[:258]
    assert_decodes(png)


@pytest.mark.parametrize("distance", [1, 2, 3, 63, 64, 65])
def test_short_periods(distance):
    png, raw = period_case(distance)
    assert len(raw) == 4 * 271
    assert_decodes(png)


@pytest.mark.parametrize("end_with_match", [False, True])
def test_length_code_edges_and_a_match_that_ends_the_image(end_with_match):
    png, raw = lengths_case(end_with_match)
    assert len(raw) == 4 * 271
    assert_decodes(png)


def junk_case():
    """A complete image, then three more literals in the same block; the trailer is the
    Adler-32 of the image's scanlines alone."""
    rng = np.random.default_rng(5)
    h, w = 3, 20
    total = h * (1 + 3 * w)
    tokens = literals(rng, 50) + [(30, 11)] + literals(rng, total - 80)
    return by_hand(h, w, tokens + [9, 8, 7], 5, adler_of=total)


def test_bytes_behind_a_complete_image_set_no_status():
    png, raw = junk_case()
    assert len(raw) == 3 * 61 + 3
    assert_decodes(png)


# ------------------------------------------------------------------ dynamic blocks at their edges
def two_valued_case():
    rng = np.random.default_rng(11)
    img = np.where(rng.integers(0, 2, (30, 40, 3)) > 0, 200, 13).astype(np.uint8)
    return pc.write_png(img, level=9)


def single_distance_code_case():
    """Literals 0..4, the end code and length 258 coded; one distance code, of one bit."""
    rng = np.random.default_rng(12)
    h, w = 4, 90
    lit = [3, 3, 3, 3, 2] + [0] * 251 + [3] + [0] * 28 + [3]
    ops = [3, 3, 3, 3, 2, (18, 138), (18, 113), 3, (18, 28), 3, 1]
    tokens = rng.integers(0, 5, 10).tolist() + [(258, 1)] + rng.integers(0, 5, 300).tolist() + [(258, 1), (258, 1)]
    tokens += rng.integers(0, 5, h * (1 + 3 * w) - 310 - 3 * 258).tolist()
    bw = pc.BitWriter()
    bw.dynamic_block(tokens, lit, [1], ops)
    raw = pc.expand(tokens)
    return pc.png_bytes(h, w, pc.zlib_wrap(bw.bytes(), raw)), raw


def crossing_repeat_case():
    """One repeat code fills the last two literal/length lengths and the first four distance lengths."""
    rng = np.random.default_rng(13)
    h, w = 4, 90
    lit = [3, 3, 3, 3] + [0] * 252 + [3] + [0] * 26 + [3, 3, 3]
    ops = [3, 3, 3, 3, (18, 138), (18, 114), 3, (18, 26), 3, (16, 6), (16, 4)]
    tokens = rng.integers(0, 4, 300).tolist() + [(258, 7), (200, 2), (230, 5)]
    tokens += rng.integers(0, 4, h * (1 + 3 * w) - 300 - 258 - 200 - 230).tolist()
    bw = pc.BitWriter()
    bw.dynamic_block(tokens, lit, [3] * 8, ops)
    raw = pc.expand(tokens)
    return pc.png_bytes(h, w, pc.zlib_wrap(bw.bytes(), raw)), raw


def test_tiny_alphabets_and_repeat_codes():
    from monodepth2_amd.png_ops import parse_png
    png = two_valued_case()
    first = pc.first_block(parse_png(png).data)
    assert first["type"] == 2 and {16, 17, 18} & set(first["cl_symbols"])
    assert sum(1 for n in first["lit_lens"][:256] if n) <= 4
    assert_decodes(png)


def test_a_single_distance_code():
    from monodepth2_amd.png_ops import parse_png
    png, raw = single_distance_code_case()
    first = pc.first_block(parse_png(png).data)
    assert first["type"] == 2 and first["dist_lens"] == [1]
    assert_decodes(png)


def test_a_repeat_across_the_alphabet_boundary():
    from monodepth2_amd.png_ops import parse_png
    png, raw = crossing_repeat_case()
    first = pc.first_block(parse_png(png).data)
    assert first["type"] == 2 and first["crossing"] and first["dist_lens"] == [3] * 8
    assert_decodes(png)


# ------------------------------------------------------------------ damage
def good_small(seed):
    rng = np.random.default_rng(seed)
    return pc.write_png(harsh(rng, 9, 13), rng.integers(0, 5, 9).tolist())


def damaged(kind):
    """(file, expected status, the file whose pixels the frame must still equal or None)."""
    rng = np.random.default_rng(21)
    h, w = 12, 17
    img = harsh(rng, h, w)
    filters = rng.integers(0, 5, h).tolist()
    raw = pc.filter_rows(img, filters)
    whole = pc.png_bytes(h, w, pc.zlib_stream(raw))
    if kind == "block_type_3":
        bw = pc.BitWriter()
        bw.fixed_block(list(raw[:100]), final=False)
        bw.block_header(3)
        bw.bits(0, 32)
        return pc.png_bytes(h, w, pc.zlib_wrap(bw.bytes(), raw)), ST_BLOCK, None
    if kind == "len_nlen":
        bw = pc.BitWriter()
        bw.stored_block(raw, nlen=(len(raw) ^ 0xFFFF) ^ 0x0100)
        return pc.png_bytes(h, w, pc.zlib_wrap(bw.bytes(), raw)), ST_BLOCK, None
    if kind == "truncated":
        z = pc.zlib_stream(raw)
        return pc.png_bytes(h, w, z[:len(z) // 2]), ST_END, None
    if kind == "distance":
        bw = pc.BitWriter()
        bw.fixed_block([1, 2, 3, (3, 10)] + list(raw[6:]))
        return pc.png_bytes(h, w, pc.zlib_wrap(bw.bytes(), raw)), ST_DIST, None
    if kind == "filter_5":
        bad = bytearray(raw)
        bad[3 * (1 + 3 * w)] = 5
        return pc.png_bytes(h, w, pc.zlib_stream(bytes(bad))), ST_FILTER, None
    if kind == "trailer":
        z = pc.zlib_stream(raw)
        return pc.png_bytes(h, w, pc.flip_bit(z, len(z) - 2, 3)), ST_ADLER, whole
    if kind == "stored_literal":
        z = pc.zlib_stream(raw, level=0)
        assert z[7:7 + len(raw)] == raw          # header 2, block header 1, LEN 2, NLEN 2
        return pc.png_bytes(h, w, pc.flip_bit(z, 7 + 2 * (1 + 3 * w) + 5, 6)), ST_ADLER, None
    if kind == "short":
        short = raw[:(h - 1) * (1 + 3 * w)]
        return pc.png_bytes(h, w, pc.zlib_stream(short)), ST_END, None
    raise ValueError(kind)


DAMAGE = ["block_type_3", "len_nlen", "truncated", "distance", "filter_5", "trailer", "stored_literal", "short"]


@pytest.mark.parametrize("kind", DAMAGE)
def test_a_damaged_file_sets_its_own_status_bit_and_nothing_else(kind):
    png, expected, still = damaged(kind)
    before, after = good_small(31), good_small(32)
    (f0, s0), (f1, s1), (f2, s2) = decode([before, png, after])
    assert s1 == expected, (s1, expected)
    assert s0 == 0 and s2 == 0
    assert np.array_equal(f0, pillow(before)) and np.array_equal(f2, pillow(after))
    if still is not None:
        assert np.array_equal(f1, pillow(still))


def test_check_names_the_first_bad_index():
    from monodepth2_amd.png_ops import decode_png_batch, parse_png
    pngs = [good_small(31), damaged("short")[0]]
    streams = [parse_png(p) for p in pngs]
    offsets, total = layout(streams)
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="stream index 1 did not decode"):
        decode_png_batch(streams, out, offsets, check=True)


# ------------------------------------------------------------------ full size
def test_a_full_size_frame_as_pillow_saves_it():
    buf = io.BytesIO()
    Image.fromarray(KT.image(np.random.default_rng(2), 375, 1242)).save(buf, "PNG")
    assert_decodes(buf.getvalue())


def test_two_runs_are_bit_equal_and_batches_mix_sizes():
    pngs = [zlib_case((66, 67), "level9"), good_small(1), zlib_case((150, 150), "rle"), longest_distance_case()[0]]
    a, b = decode(pngs), decode(pngs)
    for (fa, sa), (fb, sb), p in zip(a, b, pngs):
        assert sa == sb == 0 and np.array_equal(fa, fb) and np.array_equal(fa, pillow(p))
