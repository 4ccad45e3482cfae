"""Host side of the JPEG encoder (monodepth2_amd/jpeg_ops.py: quality_tables, jpeg_file_bytes)
and the tests' numpy restatement of the encoder's written rules (tests/jpeg_encode_case.py)
against Pillow, byte for byte: if the restatement equals Pillow's files on every case, the
rules in DESIGN.md §6k are the rules, and the GPU tests hold the kernels to the same files."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_case as jc
import jpeg_encode_case as ec
from monodepth2_amd import jpeg_ops


def same_stream(a, b):
    return ((a.height, a.width, a.sampling, tuple(map(tuple, a.factors))) ==
            (b.height, b.width, b.sampling, tuple(map(tuple, b.factors))) and
            tuple(map(tuple, a.quant)) == tuple(map(tuple, b.quant)) and a.huff == b.huff and
            tuple(a.dc) == tuple(b.dc) and tuple(a.ac) == tuple(b.ac) and a.data == b.data)


@pytest.mark.parametrize("name", list(ec.CASES))
def test_restatement_equals_pillow(name):
    _, _, _, _, samp, q = ec.CASES[name]
    s = ec.encode_np(ec.frame(name), samp, q)
    ref = ec.pillow_file(name)
    p = jpeg_ops.parse_jpeg(ref)
    assert p is not None
    assert s.quant == p.quant
    assert s.data == p.data
    assert jpeg_ops.jpeg_file_bytes(s) == ref
    assert same_stream(jpeg_ops.parse_jpeg(jpeg_ops.jpeg_file_bytes(s)), s)


def test_the_cases_cover_what_they_are_named_for():
    noise = jpeg_ops.parse_jpeg(ec.pillow_file("noise_64x96_444_q100"))
    assert b"\xff" in noise.data and len(noise.data) > 80 * 96        # about 88 bytes per block
    assert len(jpeg_ops.parse_jpeg(ec.pillow_file("flat_16x16_420_q75")).data) <= 8   # six blocks in two words
    assert 24 % 16 == 8 and 8 % 16 == 8                                # the bottom rule of 4:2:0
    assert len({ec.CASES[n][4] for n in ec.MIXED}) == 3


def test_default_save_is_quality_75_420():
    a = ec.frame("grid_37x53_420_q75")
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG")
    assert jpeg_ops.jpeg_file_bytes(ec.encode_np(a, "4:2:0", 75)) == buf.getvalue()


@pytest.mark.parametrize("quality", [1, 30, 49, 50, 75, 92, 100])
def test_quality_tables_match_pillow(quality):
    p = jpeg_ops.parse_jpeg(jc.encode(jc.textured(16, 16, 3), "4:2:0", quality))
    luma, chroma = jpeg_ops.quality_tables(quality)
    assert (luma, chroma, chroma) == p.quant


def test_quality_range():
    for q in (0, 101, -3):
        with pytest.raises(ValueError):
            jpeg_ops.quality_tables(q)


def test_standard_tables_are_pillows():
    p = jpeg_ops.parse_jpeg(jc.encode(jc.textured(16, 16, 3)))
    assert p.huff == jpeg_ops.STD_HUFF


@pytest.mark.parametrize("name", ["size_17x33_420", "mix_24x40_422_q30_opt", "noise_64x96_q100_444"])
def test_file_bytes_round_trip_of_a_parsed_file(name):
    """any supported stream, optimised tables included: parse(file_bytes(s)) gives back s"""
    s = jc.parsed(name)
    again = jpeg_ops.parse_jpeg(jpeg_ops.jpeg_file_bytes(s))
    assert again is not None and same_stream(again, s)
    if "opt" not in name:
        assert jpeg_ops.jpeg_file_bytes(s) == jc.cases()[name]


def test_file_bytes_refuses_what_the_layout_cannot_hold():
    s = jc.parsed("size_16x16_420")

    def variant(**kw):
        f = {k: getattr(s, k) for k in jpeg_ops.JpegStream.__slots__}
        f.update(kw)
        return jpeg_ops.JpegStream(**f)

    with pytest.raises(ValueError, match="sampling factors"):
        jpeg_ops.jpeg_file_bytes(variant(factors=((1, 2), (1, 1), (1, 1))))
    with pytest.raises(ValueError, match="sampling factors"):
        jpeg_ops.jpeg_file_bytes(variant(factors=((2, 2), (2, 1), (1, 1))))
    other = tuple(min(v + 1, 255) for v in s.quant[2])
    with pytest.raises(ValueError, match="different quantisation"):
        jpeg_ops.jpeg_file_bytes(variant(quant=(s.quant[0], s.quant[1], other)))
    huff = dict(s.huff)
    huff[(1, 2)] = huff[(1, 0)]
    with pytest.raises(ValueError, match="different Huffman"):
        jpeg_ops.jpeg_file_bytes(variant(huff=huff, ac=(0, 1, 2)))


def test_sampling_names():
    for name, cls in (("4:4:4", 0), ("422", 1), (420, 2), ("4:2:0", 2), (1, 1)):
        assert jpeg_ops.sampling_class(name) == cls
    with pytest.raises(ValueError):
        jpeg_ops.sampling_class("4:1:1")
