"""tests/png_encode_case.py (the PNG encoder's rules) held to the PNG and zlib
standards on the CPU: Pillow opens every file the restatement writes, zlib inflates its IDAT
payload to the filtered scanlines, every segment starts where the rules say and inflates on
its own, and the sizes stay under the bound and under the ratios DESIGN.md §6n records."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_encode_case as ec

CASES = ec.cases()
SINGLE = [k for k in CASES if k != "mixed_batch"]
_info = {}


def info_of(name, i=0):
    if (name, i) not in _info:
        frame, kind, s = CASES[name][i]
        _info[(name, i)] = ec.encode_info(frame, kind, s)
    return _info[(name, i)]


ALL = [(name, i) for name in CASES for i in range(len(CASES[name]))]


def idat_of(data):
    assert data[:8] == ec.SIGNATURE
    pos, out, kinds = 8, b"", []
    while pos < len(data):
        (n,) = struct.unpack_from(">I", data, pos)
        kind = data[pos + 4:pos + 8]
        assert zlib.crc32(data[pos + 4:pos + 8 + n]) == struct.unpack_from(">I", data, pos + 8 + n)[0]
        kinds.append(kind)
        if kind == b"IDAT":
            out += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    assert kinds == [b"IHDR", b"IDAT", b"IEND"]
    return out


@pytest.mark.parametrize("name,i", ALL)
def test_pillow_reads_the_file(name, i):
    frame, kind, _ = CASES[name][i]
    im = Image.open(io.BytesIO(info_of(name, i)["file"]))
    im.load()
    h, w = frame.shape[:2]
    assert im.size == (w, h)
    if kind == ec.RGB8:
        assert im.mode == "RGB"
        assert np.array_equal(np.asarray(im), frame)
    else:
        assert im.mode in ("I;16", "I;16B", "I")
        assert np.array_equal(np.asarray(im).astype(np.uint16), np.asarray(frame).view(np.uint16))


@pytest.mark.parametrize("name,i", ALL)
def test_zlib_inflates_to_the_filtered_scanlines(name, i):
    info = info_of(name, i)
    z = idat_of(info["file"])
    assert z == info["zstream"]
    assert zlib.decompress(z) == info["filtered"]
    assert len(z) <= ec.encode_bound(info["height"], info["width"], info["kind"], info["segment_bytes"])
    assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(info["filtered"])


@pytest.mark.parametrize("name,i", ALL)
def test_segments_start_where_the_rules_say(name, i):
    info = info_of(name, i)
    d, s, z = info["filtered"], info["segment_bytes"], info["zstream"]
    segs = info["segments"]
    assert len(segs) == -(-len(d) // s)
    pos = 2
    for k, seg in enumerate(segs):
        assert (seg["start"], seg["end"]) == (k * s, min(len(d), (k + 1) * s))
        assert seg["offset"] == pos
        pos += seg["nbytes"]
        body = z[seg["offset"]:seg["offset"] + seg["nbytes"]]
        last = k == len(segs) - 1
        if not last:
            assert body[-4:] == b"\x00\x00\xff\xff"
        # the segment inflates on its own, given the input before it as the window
        o = zlib.decompressobj(-15, zdict=d[max(0, seg["start"] - 32768):seg["start"]]) if seg["start"] else \
            zlib.decompressobj(-15)
        assert o.decompress(body) == d[seg["start"]:seg["end"]]
        assert o.eof == last
        for t in seg["tokens"]:
            if isinstance(t, tuple):
                assert 3 <= t[0] <= 258 and 1 <= t[1] <= 32768
    assert pos + 4 == len(z)


def test_each_filter_wins_a_row():
    assert info_of("filters_5rows_rgb")["filters"] == [0, 1, 2, 3, 4]


def test_a_tie_goes_to_the_lowest_filter():
    frame, kind, _ = CASES["tie_rows"][0]
    rows = ec.raw_rows(frame, kind)
    r = ec.residuals(rows, 3).astype(np.int64)
    cost = np.where(r < 128, r, 256 - r).sum(axis=2)
    assert cost[1, 0] == cost[4, 0] < cost[0, 0]          # Sub and Paeth tie on row 0
    assert cost[2, 1] == cost[4, 1] < cost[1, 1]          # Up and Paeth tie on row 1
    assert info_of("tie_rows")["filters"] == [1, 2]


def test_flat_runs_one_distance_code_and_a_one_literal_block():
    segs = info_of("flat_40x70_rgb")["segments"]
    tokens = [t for s in segs for t in s["tokens"]]
    assert sum(1 for t in tokens if t == (258, 1)) >= 20
    assert all(s["dist_symbols"] == 1 and not s["stored"] for s in segs)
    assert tokens[0] == 0 and all(t == (258, 1) for t in tokens[1:-1])    # one literal, then the runs


def test_one_literal_and_end_of_block_only():
    # a segment of zeros behind zeros: its first byte is already inside a match's reach, so
    # the block may hold one literal (or none) beside lengths and the end of block
    info = ec.encode_info(np.zeros((3, 400, 3), np.uint8), ec.RGB8, 1024)
    assert zlib.decompress(info["zstream"]) == info["filtered"]
    one = ec.encode_info(np.zeros((1, 1, 3), np.uint8), ec.RGB8, 1024)      # 4 bytes: stored
    assert one["segments"][0]["stored"]
    lit = [0] * 286
    lit[65], lit[256] = 5, 1
    assert ec.code_lengths(lit, 15)[65] == 1 and ec.code_lengths(lit, 15)[256] == 1
    assert ec.code_lengths([0] * 30, 15)[:3] == [1, 1, 0]
    assert ec.code_lengths([0, 0, 0, 9] + [0] * 26, 15)[:4] == [1, 0, 0, 1]


def test_noise_is_stored_with_no_match():
    segs = info_of("noise_32x48_rgb")["segments"]
    assert len(segs) > 1 and all(s["stored"] for s in segs)
    assert not any(isinstance(t, tuple) for s in segs for t in s["tokens"])


def test_edge_geometries():
    for name, nseg in (("edge_exact_S", 1), ("edge_S_minus_1", 1), ("edge_S_plus_1", 2), ("edge_3S_plus_7", 4)):
        assert len(info_of(name)["segments"]) == nseg, name
    info = info_of("row_straddles_cut")
    assert 1024 % (1 + 3 * info["width"]) != 0
    segs = info_of("match_from_previous_segment")["segments"]
    reach = [seg["start"] - (p - t[1]) for seg in segs[1:] for p, t in _positions(seg) if isinstance(t, tuple)]
    assert max(reach) > 0                                  # a match's source starts before its segment


def _positions(seg):
    p = seg["start"]
    for t in seg["tokens"]:
        yield p, t
        p += t[0] if isinstance(t, tuple) else 1


def test_length_limit_rule():
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    lens = ec.code_lengths(fib + [0] * 6, 15)
    assert max(lens) <= 15 and sum(2.0 ** -n for n in lens if n) == 1.0
    lens = ec.code_lengths(fib[:19], 7)
    assert max(lens) <= 7 and sum(2.0 ** -n for n in lens if n) == 1.0


# ours / Pillow's save() of the same array, measured with this restatement
RATIO = {
    "flat_40x70_rgb": 1.0000,
    "depth_like_64x96_gray16": 1.2539,
    "panel_like_48x160_rgb": 0.9529,
    "match_from_previous_segment": 1.4095,
    "edge_3S_plus_7": 1.6250,
    "row_straddles_cut": 1.1441,
}


def _pillow_size(frame, kind):
    buf = io.BytesIO()
    Image.fromarray(np.asarray(frame).view(np.uint16) if kind == ec.GRAY16 else frame).save(buf, "PNG")
    return len(buf.getvalue())


@pytest.mark.parametrize("name", ec.COMPRESSIBLE)
def test_compression_against_pillow(name):
    frame, kind, s = CASES[name][0]
    info = info_of(name)
    ours, theirs = len(info["file"]), _pillow_size(frame, kind)
    print(f"{name}: ours {ours} Pillow {theirs} ratio {ours / theirs:.4f}")
    assert ours <= RATIO[name] * 1.10 * theirs
    stored = len(info["filtered"]) + 10 * len(info["segments"]) + 6 + (len(info["file"]) - len(info["zstream"]))
    assert ours < stored
