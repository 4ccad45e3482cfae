"""The PNG test helper (tests/png_case.py) against Pillow and zlib, and png_ops.parse_png on
the files it must take and the ones it must leave to PIL — all on the CPU."""
import io
import os
import zlib

import numpy as np
import pytest
from PIL import Image

import kitti_tree as KT
import png_case as pc
from monodepth2_amd.png_ops import PngStream, parse_png


def pillow(png):
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))


def image(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def inflate(stream):
    """The scanlines of a PngStream: zlib's own answer for the zlib stream it came from."""
    return zlib.decompress(b"\x78\x9c" + stream.data)


def save(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG", **kw)
    return buf.getvalue()


# ------------------------------------------------------------------ the helper itself
@pytest.mark.parametrize("filt", [pc.NONE, pc.SUB, pc.UP, pc.AVG, pc.PAETH, "mixed"])
def test_the_writer_round_trips_through_pillow_and_zlib(filt):
    rng = np.random.default_rng(3)
    img = image(13, 9, 1)
    img[rng.integers(0, 3, img.shape) == 0] = 0
    img[rng.integers(0, 3, img.shape) == 0] = 255
    filters = rng.integers(0, 5, 13).tolist() if filt == "mixed" else [filt] * 13
    for kw in (dict(), dict(level=0), dict(level=9, strategy=zlib.Z_RLE), dict(wbits=9),
               dict(flush_every=100, flush_mode=zlib.Z_SYNC_FLUSH), dict(splits=(1, 0, 1, 3))):
        png = pc.write_png(img, filters, **kw)
        assert np.array_equal(pillow(png), img)
        s = parse_png(png)
        assert inflate(s) == pc.filter_rows(img, filters)
        assert [inflate(s)[r * 28] for r in range(13)] == filters


def test_the_bit_writer_round_trips_through_zlib_and_pillow():
    rng = np.random.default_rng(4)
    h, w = 4, 90
    tokens = rng.integers(0, 256, 400).tolist() + [(3, 1), (258, 400), (10, 7), (11, 64), (257, 3), (30, 300)]
    tokens += rng.integers(0, 256, h * 271 - 400 - 569).tolist()
    tokens = pc.settle_filter_bytes(tokens, 271, rng)
    raw = pc.expand(tokens)
    assert len(raw) == h * 271 and all(raw[r * 271] <= 4 for r in range(h))
    bw = pc.BitWriter()
    bw.fixed_block(tokens[:500], final=False)
    bw.stored_block(b"", final=False)
    bw.fixed_block(tokens[500:])
    z = pc.zlib_wrap(bw.bytes(), raw)
    assert zlib.decompress(z) == raw
    png = pc.png_bytes(h, w, z)
    assert pillow(png).shape == (h, w, 3)
    assert inflate(parse_png(png)) == raw
    # a stored block by hand, and a dynamic one with a single distance code
    bw = pc.BitWriter()
    bw.stored_block(raw[:300], final=False)
    bw.stored_block(raw[300:])
    assert zlib.decompress(pc.zlib_wrap(bw.bytes(), raw)) == raw
    lit = [3, 3, 3, 3, 2] + [0] * 251 + [3] + [0] * 28 + [3]
    toks = [0, 1, 2, 3, 4, (258, 1), 4, 4]
    bw = pc.BitWriter()
    bw.dynamic_block(toks, lit, [1], [3, 3, 3, 3, 2, (18, 138), (18, 113), 3, (18, 28), 3, 1])
    assert zlib.decompress(pc.zlib_wrap(bw.bytes(), pc.expand(toks))) == pc.expand(toks)
    first = pc.first_block(bw.bytes())
    assert first["type"] == 2 and first["dist_lens"] == [1] and first["lit_lens"] == lit and not first["crossing"]


def test_first_block_reads_zlibs_headers():
    raw = pc.filter_rows(KT.image(np.random.default_rng(2), 20, 30), [pc.SUB] * 20)
    assert pc.first_block(pc.zlib_stream(raw, level=0)[2:])["type"] == 0
    assert pc.first_block(pc.zlib_stream(raw, strategy=zlib.Z_FIXED)[2:])["type"] == 1
    first = pc.first_block(pc.zlib_stream(raw, level=9)[2:])
    assert first["type"] == 2 and first["final"] == 1 and len(first["lit_lens"]) == first["nlen"] >= 257


# ------------------------------------------------------------------ parse_png accepts
def check_accepted(png, img):
    s = parse_png(png)
    assert isinstance(s, PngStream)
    assert (s.height, s.width) == img.shape[:2] and s.size == (img.shape[1], img.shape[0])
    raw = inflate(s)
    assert len(raw) == s.height * (1 + 3 * s.width)
    assert np.array_equal(pillow(png), img)
    return s


def test_every_file_of_the_synthetic_tree(tmp_path):
    written = KT.write_tree(str(tmp_path), ext=".png")
    assert len(written) == 12
    for rel, arr in written.items():
        with open(os.path.join(str(tmp_path), rel), "rb") as f:
            check_accepted(f.read(), arr)


@pytest.mark.parametrize("kw", [dict(compress_level=0), dict(compress_level=9), dict(optimize=True)],
                         ids=["level0", "level9", "optimize"])
def test_pillows_own_saves(kw):
    img = KT.image(np.random.default_rng(5), 37, 53)
    check_accepted(save(img, **kw), img)


def test_idat_split_anywhere():
    img = image(9, 7)
    whole = pc.write_png(img, [pc.PAETH] * 9)
    split = pc.write_png(img, [pc.PAETH] * 9, splits=(1, 1, 3))
    assert split.count(b"IDAT") == 4
    assert check_accepted(split, img).data == check_accepted(whole, img).data
    empty = pc.write_png(img, [pc.PAETH] * 9, splits=(0, 2, 0))
    assert check_accepted(empty, img).data == parse_png(whole).data


def test_a_trns_chunk_on_an_rgb_file_changes_nothing():
    img = image(6, 5)
    img[2, 3] = (1, 2, 3)
    png = pc.write_png(img, extra=[pc.chunk(b"tRNS", bytes([0, 1, 0, 2, 0, 3]))])
    assert b"tRNS" in png
    check_accepted(png, img)
    check_accepted(pc.write_png(img, extra=[pc.chunk(b"gAMA", (45455).to_bytes(4, "big")), pc.chunk(b"tEXt", b"a\0b")]),
                   img)


def test_a_small_window_in_the_zlib_header():
    img = image(8, 8)
    png = pc.write_png(img, wbits=9)
    i = png.index(b"IDAT") + 4
    assert png[i] >> 4 == 1 and png[i] & 15 == 8     # CINFO 1: a 512-byte window
    check_accepted(png, img)


# ------------------------------------------------------------------ parse_png refuses
def test_other_pixel_formats():
    rng = np.random.default_rng(6)
    gray = rng.integers(0, 256, (8, 9), dtype=np.uint8)
    assert parse_png(save(gray)) is None
    assert parse_png(save((rng.integers(0, 65536, (8, 9))).astype(np.uint16))) is None
    buf = io.BytesIO()
    Image.fromarray(image(8, 9)).convert("P").save(buf, "PNG")
    assert parse_png(buf.getvalue()) is None
    assert parse_png(save(rng.integers(0, 256, (8, 9, 4), dtype=np.uint8))) is None


def test_interlaced():
    img = image(8, 9)
    z = pc.zlib_stream(pc.filter_rows(img, [0] * 8))
    png = b"".join([pc.SIGNATURE, pc.ihdr(8, 9, interlace=1), pc.chunk(b"IDAT", z), pc.chunk(b"IEND")])
    assert parse_png(png) is None
    assert parse_png(png.replace(pc.ihdr(8, 9, interlace=1), pc.ihdr(8, 9))) is not None


def test_damaged_containers():
    img = image(8, 9)
    png = pc.write_png(img)
    assert parse_png(png) is not None
    assert parse_png(pc.flip_crc_bit(png)) is None
    assert parse_png(pc.without_iend(png)) is None
    assert parse_png(png[:-1]) is None
    z = pc.zlib_stream(pc.filter_rows(img, [0] * 8))
    wide = b"".join([pc.SIGNATURE, pc.ihdr(8, 8193), pc.chunk(b"IDAT", z), pc.chunk(b"IEND")])
    assert parse_png(wide) is None
    assert parse_png(b"".join([pc.SIGNATURE, pc.ihdr(8, 8192), pc.chunk(b"IDAT", z), pc.chunk(b"IEND")])) is not None
    assert parse_png(b"".join([pc.SIGNATURE, pc.ihdr(0, 9), pc.chunk(b"IDAT", z), pc.chunk(b"IEND")])) is None
    # no IDAT at all, two runs of IDAT, an unknown critical chunk, APNG
    assert parse_png(b"".join([pc.SIGNATURE, pc.ihdr(8, 9), pc.chunk(b"IEND")])) is None
    two = b"".join([pc.SIGNATURE, pc.ihdr(8, 9), pc.chunk(b"IDAT", z[:5]), pc.chunk(b"tEXt", b"a\0b"),
                    pc.chunk(b"IDAT", z[5:]), pc.chunk(b"IEND")])
    assert parse_png(two) is None
    assert parse_png(pc.write_png(img, extra=[pc.chunk(b"ABCD", b"x")])) is None
    assert parse_png(pc.write_png(img, extra=[pc.chunk(b"acTL", bytes(8))])) is None
    # zlib headers the decoder does not take: a preset dictionary, a bad check, another method
    for header in (b"\x78\xbb", b"\x78\x9d", b"\x79\x9c", b"\x88\x1c"):
        assert parse_png(pc.png_bytes(8, 9, header + z[2:])) is None


def test_files_that_are_not_png():
    buf = io.BytesIO()
    Image.fromarray(image(8, 9)).save(buf, "JPEG")
    png = pc.write_png(image(8, 9))
    for data in (buf.getvalue(), b"", b"\x89PNG", png[:20], png[:8], bytearray(png[:30]), b"\0" * 100):
        assert parse_png(data) is None
    assert parse_png(bytearray(png)) is not None and parse_png(memoryview(png)) is not None
