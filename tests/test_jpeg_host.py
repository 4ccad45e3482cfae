"""CPU-side checks of the JPEG path's host half (monodepth2_amd/jpeg_ops.py) and of the
tests' numpy restatement of the decoder (tests/jpeg_case.py): the restatement is
byte-identical to Pillow on every case, so the rules the kernels follow are pinned here;
`parse_jpeg` takes exactly the supported class; the fixed-point synchronisation of the
entropy decoder equals the sequential decode."""
import io

import numpy as np
import pytest
from PIL import Image

from monodepth2_amd import jpeg_ops
from monodepth2_amd.jpeg_ops import ZIGZAG, parse_jpeg, unstuff

import jpeg_case as jc


@pytest.mark.parametrize("name", list(jc.cases()))
def test_restatement_is_byte_identical_to_pillow(name):
    out = jc.decode_np(jc.parsed(name))
    ref = jc.pillow_rgb(name)
    assert out.shape == ref.shape and out.dtype == ref.dtype
    assert np.array_equal(out, ref), int(np.abs(out.astype(int) - ref).max())


def pil_bytes(mode="RGB", fmt="JPEG", size=(40, 24), **kw):
    arr = jc.textured(size[1], size[0], 5)
    img = Image.fromarray(arr)
    if mode != "RGB":
        img = img.convert(mode)
    buf = io.BytesIO()
    img.save(buf, fmt, **kw)
    return buf.getvalue()


def test_unsupported_files_parse_to_none():
    assert parse_jpeg(pil_bytes(progressive=True)) is None
    assert parse_jpeg(pil_bytes(mode="L")) is None
    assert parse_jpeg(pil_bytes(mode="CMYK")) is None
    restart = pil_bytes(restart_marker_blocks=4)
    assert b"\xff\xdd" in restart            # Pillow wrote a DRI segment
    assert parse_jpeg(restart) is None
    assert parse_jpeg(pil_bytes(fmt="PNG")) is None
    good = pil_bytes()
    assert parse_jpeg(good) is not None
    assert parse_jpeg(good[:-2]) is None      # cut before EOI
    assert parse_jpeg(good[:len(good) // 2]) is None
    assert parse_jpeg(good[:10]) is None and parse_jpeg(b"") is None
    assert parse_jpeg(memoryview(good)) is not None


def test_markers_that_change_the_colour_space_are_refused():
    good = pil_bytes()
    sof = good.index(b"\xff\xc0")
    ids = bytearray(good)
    for i, ch in enumerate(b"RGB"):           # component ids R, G, B: libjpeg decodes as RGB
        ids[sof + 10 + 3 * i] = ch
    sos = good.index(b"\xff\xda")
    for i, ch in enumerate(b"RGB"):
        ids[sos + 5 + 2 * i] = ch
    assert parse_jpeg(bytes(ids)) is None
    adobe = b"\xff\xee" + (14).to_bytes(2, "big") + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1])
    assert parse_jpeg(good[:2] + adobe + good[2:]) is None
    twelve = bytearray(good)
    twelve[sof + 4] = 12
    assert parse_jpeg(bytes(twelve)) is None
    big = bytearray(good)
    big[sof + 5:sof + 7] = (8193).to_bytes(2, "big")
    assert parse_jpeg(bytes(big)) is None
    dri = b"\xff\xdd\x00\x04\x00\x00"         # a zero interval is no restart interval
    assert parse_jpeg(good[:2] + dri + good[2:]) is not None
    assert parse_jpeg(good[:2] + dri[:-1] + b"\x08" + good[2:]) is None


@pytest.mark.parametrize("name", ["size_17x33_444", "size_37x53_422", "size_37x53_420", "mix_24x40_420_q30_opt",
                                  "mix_24x40_422_q100", "size_1x1_420"])
def test_parsed_description_agrees_with_pillow(name):
    data = jc.cases()[name]
    s = parse_jpeg(data)
    img = Image.open(io.BytesIO(data))
    assert s.size == img.size and (s.width, s.height) == img.size
    assert img.layers == 3 and len(s.quant) == 3
    assert {"444": 0, "422": 1, "420": 2}[name.split("_")[2]] == s.sampling
    assert s.factors[1] == s.factors[2] == (1, 1)
    q = img.quantization                      # table id -> 64 values, which Pillow has de-zigzagged
    tables = [q[0], q[1], q[1]] if len(q) > 1 else [q[0]] * 3
    dqt = data.index(b"\xff\xdb")             # the file's first table, in the zigzag order of the segment
    zz = list(data[dqt + 5:dqt + 69])
    assert [s.quant[0][ZIGZAG[k]] for k in range(64)] == zz
    for c in range(3):
        assert list(s.quant[c]) == list(tables[c])
    for (cls, tid), (counts, vals) in s.huff.items():
        assert cls in (0, 1) and len(counts) == 16 and sum(counts) == len(vals)
    assert set(s.huff) == {(0, t) for t in s.dc} | {(1, t) for t in s.ac}
    start = data.index(b"\xff\xda")
    start += 2 + int.from_bytes(data[start + 2:start + 4], "big")
    assert s.data == data[start:-2].replace(b"\xff\x00", b"\xff")


def test_unstuffing():
    assert unstuff(b"\x12\xff\x00\x00\x34") == b"\x12\xff\x00\x34"        # FF 00 00: one pair only
    assert unstuff(b"\xff\x00\xff\x00") == b"\xff\xff"
    assert unstuff(b"\x00\xff\x00") == b"\x00\xff"
    assert unstuff(b"") == b""
    # a file whose entropy segment holds FF 00 00 keeps the zero byte that follows the pair
    good = jc.cases()["noise_64x96_q100_444"]
    s = parse_jpeg(good)
    start = good.index(b"\xff\xda")
    start += 2 + int.from_bytes(good[start + 2:start + 4], "big")
    assert good.count(b"\xff\x00", start) > 0
    assert len(s.data) == len(good) - 2 - start - good.count(b"\xff\x00", start)


def test_huffman_table_check():
    ok = jpeg_ops._huffman_ok
    assert ok((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), 12)     # the standard luminance DC table
    assert not ok((2,) + (0,) * 15, 2)                                   # the all-ones code of length 1
    assert not ok((0, 5) + (0,) * 14, 5)                                 # oversubscribed
    assert not ok((0, 1) + (0,) * 14, 2)                                 # values and counts disagree


@pytest.mark.parametrize("name", ["noise_64x96_q100_444", "mix_24x40_422_q92_opt"])
def test_fixed_point_equals_the_sequential_decode(name):
    s = jc.parsed(name)
    slots, counts, rounds, decodes, E = jc.fixed_point_slots(s)
    _, done, boundaries, _ = jc.sequential_coefficients(s)
    print(name, "subsequences", E.nsub, "rounds", rounds, "decodes", decodes)
    assert slots[:E.nsub] == boundaries
    assert sum(counts) == done == E.total_blocks
    assert rounds <= E.nsub + 1


def test_describe_batch_deduplicates_tables_and_lays_out_streams():
    names = ["size_17x33_444", "size_37x53_422", "mix_24x40_420_q92", "mix_24x40_420_q92_opt", "mix_24x40_444_q30"]
    streams = [jc.parsed(n) for n in names]
    images, quant, huff, base, total = jpeg_ops.describe_batch(streams, [i * 16384 for i in range(len(names))])
    assert len(quant) == 4                    # q92 luma / chroma shared by four files, q30's own two
    assert len(huff) == 4 + 4                 # the standard four, and the optimised file's own
    assert base % 16 == 0 and base >= len(quant) * 128 + len(huff) * 272
    for i, s in enumerate(streams):
        im = images[i]
        assert (im.height, im.width, im.sampling, im.stream_bytes) == (s.height, s.width, s.sampling, len(s.data))
        assert im.stream_offset % 16 == 0 and im.out_offset == i * 16384
        assert quant[im.quant[0]] == s.quant[0] and huff[im.ac[2]] == s.huff[(1, s.ac[2])]
    host = np.zeros(total, np.uint8)
    jpeg_ops.fill_staging(host, streams, images, quant, huff, base)
    o = base + images[3].stream_offset
    assert bytes(host[o:o + len(streams[3].data)]) == streams[3].data
    with pytest.raises(ValueError, match="offsets"):
        jpeg_ops.describe_batch(streams, [0])


def test_decode_has_no_cpu_fallback():
    import torch
    s = jc.parsed("size_8x8_444")
    with pytest.raises(RuntimeError, match="GPU only"):
        jpeg_ops.decode_jpeg_batch([s], torch.zeros(256, dtype=torch.uint8), [0], device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        jpeg_ops.decode_jpeg_batch([s], torch.zeros(256, dtype=torch.uint8), [0])
