"""Host-side checks of the PNG segment index, no GPU: the pure-Python
restatement of the segment rule (tests/png_index_case.py) against zlib on every stream the
GPU tests use, the S..S + 257 rule, the conditions that keep the GPU tests from passing
vacuously, and KIND_PNG records through write_pack / FramePack with restatement-made indexes."""
import struct
import zlib

import numpy as np
import pytest

import png_case as pc
import png_index_case as pic

S = pic.S


def all_cases():
    cases = dict(pic.library_cases())
    cases.update(pic.handmade_cases())
    cases["far"] = pic.far_case()
    for i, png in enumerate(pic.mixed_batch()):
        cases["mixed%d" % i] = png
    return cases


@pytest.fixture(scope="module")
def walked():
    """{name: (PngStream, index bytes, Walk)} at S = 1024, made once; every index as long as
    the package says an index of its geometry is."""
    from monodepth2_amd.png_ops import index_nbytes, parse_png
    out = {}
    for name, png in all_cases().items():
        s = parse_png(png)
        assert s is not None, name
        out[name] = (s,) + pic.index_of(s, S)
        assert len(out[name][1]) == index_nbytes(s.height, s.width, S), name
    return out


def test_the_restatement_inflates_what_zlib_inflates(walked):
    for name, (s, _, w) in walked.items():
        total = s.height * (1 + 3 * s.width)
        want = zlib.decompressobj(-15).decompress(s.data[:-4])
        assert w.out == want[:total] and len(want) >= total, name
        assert struct.unpack(">I", s.data[-4:])[0] == zlib.adler32(w.out), name


def test_segments_hold_s_to_s_plus_257_bytes(walked):
    for name, (s, index, w) in walked.items():
        total = s.height * (1 + 3 * s.width)
        assert w.entries[0] == (0, 0, 0)
        starts = [e[2] for e in w.entries] + [total]
        sizes = [b - a for a, b in zip(starts, starts[1:])]
        assert all(S <= n <= S + 257 for n in sizes[:-1]) and 0 < sizes[-1] <= S + 257, (name, sizes)
        assert len(w.entries) <= total // S + 1
        assert all(hb <= sb <= 8 * (len(s.data) - 4) for hb, sb, _ in w.entries), name
        assert pic.read_index(index) == (len(w.entries), S, w.entries)


def test_the_cases_cannot_pass_vacuously(walked):
    """every multi-segment case has at least 3 segments; every hand-made one has bytes whose
    source lies in an earlier segment; each names what it was made for"""
    for name, (s, _, w) in walked.items():
        if s.height * (1 + 3 * s.width) > S:
            assert len(w.entries) >= 3, (name, len(w.entries))
    for name in list(pic.handmade_cases()) + ["far"]:
        s, _, w = walked[name]
        assert len(w.entries) >= 3 and w.crossing >= 1, (name, len(w.entries), w.crossing)
    assert walked["chain_through_segments"][2].depth >= 2        # segment 3 <- 2 <- 1
    assert walked["period_from_before_boundary"][2].crossing == 120   # 3 of the 5 period bytes lie before 1024
    # a match at distance 32768 from a segment's first byte
    s, _, w = walked["far"]
    assert (33 * 1024) in [e[2] for e in w.entries] and w.out[33 * 1024:33 * 1024 + 100] == w.out[1024:1124]
    # one block spanning the image: every entry but the first is mid-block
    for name, kind in (("one_dynamic_block", 2), ("one_fixed_block", 1)):
        s, _, w = walked[name]
        assert pc.first_block(s.data)["type"] == kind and pc.first_block(s.data)["final"] == 1
        assert all(hb == 0 and sb > 3 for hb, sb, _ in w.entries[1:])
    # a stored block cut by boundaries: entries whose symbol is a byte of the block
    s, _, w = walked["stored_block_cut"]
    assert pc.first_block(s.data)["type"] == 0
    inside = [e for e in w.entries[1:] if e[0] == 0]
    assert len(inside) >= 2 and all(sb % 8 == 0 and sb // 8 == 5 + op for _, sb, op in inside)
    # flushes put empty stored blocks on and next to boundaries.  In a Huffman block the end-of-
    # block symbol at the boundary is the candidate (the empty block follows the entry); behind
    # a stored block that ends on the boundary it is the empty block's header itself
    for name in ("zlib_sync_flush", "zlib_full_flush"):
        s, _, w = walked[name]
        assert [op for _, _, op in w.entries] == list(range(0, 8 * 1024, 1024)), name
        assert all(hb < sb for hb, sb, _ in w.entries[1:]), name
    assert all(hb == sb for hb, sb, _ in walked["zlib_level0_flush"][2].entries[1:])
    assert all(hb < sb and sb % 8 == 0 for hb, sb, _ in walked["zlib_level0_flush_near"][2].entries[1:])
    assert len(walked["1x1"][2].entries) == 1 and len(walked["1x8192"][2].entries) >= 3


@pytest.mark.parametrize("size", [(1, 1), (24, 100), (375, 1242), (8192, 8192), (1, 341), (3, 341)])
@pytest.mark.parametrize("segment_bytes", [1024, 16384, 32768])
def test_index_nbytes_is_fixed_per_geometry(size, segment_bytes):
    from monodepth2_amd.png_ops import index_nbytes
    h, w = size
    assert index_nbytes(h, w, segment_bytes) == pic.index_nbytes(h, w, segment_bytes)
    assert index_nbytes(h, w, segment_bytes) % 16 == 0
    assert index_nbytes(h, w, segment_bytes) >= 16 + 24 * (h * (1 + 3 * w) // segment_bytes + 1)


@pytest.mark.parametrize("bad", [0, 512, 1000, 3000, 65536, -1024])
def test_a_bad_segment_bytes_is_refused(bad):
    from monodepth2_amd.png_ops import index_nbytes
    with pytest.raises(ValueError, match="power of two in 1024..32768"):
        index_nbytes(24, 100, bad)


# ------------------------------------------------------------------ packs
PARENT_PACK = (590000, "62d54c2fa86d152922f18ba507c6f799a282a91586c56a8c3f4cc90d1817239c")


def jpeg_and_raw_records():
    """The records of test_pack_format.py's fixture: every JPEG case with its restated index
    and two RAW frames.  The writer before PNG records existed gave PARENT_PACK (bytes,
    SHA-256) for them in this order."""
    import jpeg_case as jc
    import jpeg_index_case as ic
    from monodepth2_amd.pack import PackRecord
    recs = [PackRecord("cases/{}.jpg".format(name), stream=jc.parsed(name), index=ic.restated_bytes(name))
            for name in jc.cases()]
    rng = np.random.RandomState(3)
    recs.append(PackRecord("raw/odd_7x5.png", raw=rng.randint(0, 256, (7, 5, 3)).astype(np.uint8)))
    recs.append(PackRecord("raw/one_1x1.png", raw=rng.randint(0, 256, (1, 1, 3)).astype(np.uint8)))
    return recs


def png_records(walked, names=("pillow_6", "zlib_sync_flush", "one_dynamic_block", "1x1")):
    from monodepth2_amd.pack import PackRecord
    return [PackRecord("png/%s.png" % n, stream=walked[n][0], index=walked[n][1]) for n in names]


def test_png_records_round_trip(walked, tmp_path):
    from monodepth2_amd.pack import KIND_PNG, FramePack, write_pack
    from monodepth2_amd.png_ops import index_nbytes
    path = str(tmp_path / "a.pack")
    recs = png_records(walked) + jpeg_and_raw_records()
    assert write_pack(path, recs) == len(recs)
    fp = FramePack(path)
    assert fp.png_segment_bytes == S
    for rec in png_records(walked):
        row = fp.record(rec.name)
        s, index = fp.png_stream(rec.name)
        assert row["kind"] == KIND_PNG == 2 and row["sampling"] == S
        assert not row["quant"].any() and not row["dc"].any() and not row["ac"].any() and not row["reserved"].any()
        assert (s.height, s.width, s.data) == (rec.stream.height, rec.stream.width, rec.stream.data)
        assert np.array_equal(index, rec.index)
        assert row["stream_bytes"] == len(s.data)
        assert row["data_bytes"] == (len(s.data) + 15) // 16 * 16 + index_nbytes(s.height, s.width, S)
        assert row["data_offset"] % 16 == 0
        with pytest.raises(ValueError, match="PNG record"):
            fp.stream(rec.name)
    other = [r.name for r in jpeg_and_raw_records()][0]
    with pytest.raises(ValueError, match="record"):
        fp.png_stream(other)
    fp.close()


def test_a_record_that_disagrees_with_its_geometry_is_a_pack_error(walked, tmp_path):
    from monodepth2_amd.pack import RECORD, FramePack, PackError, PackRecord, write_pack, _HEADER
    path = str(tmp_path / "b.pack")
    write_pack(path, png_records(walked))
    with open(path, "rb") as f:
        data = bytearray(f.read())
    rec_off = _HEADER.unpack_from(data)[9]
    for field, delta in (("data_bytes", -16), ("height", 60), ("stream_bytes", 32), ("sampling", 1024)):
        bad = bytearray(data)
        table = np.frombuffer(bad, RECORD, 4, rec_off)
        table[field][2] = int(table[field][2]) + delta
        p = str(tmp_path / ("bad_%s.pack" % field))
        with open(p, "wb") as f:
            f.write(bad)
        with pytest.raises(PackError):
            FramePack(p)
    # the writer refuses an index of the wrong size before anything is written
    s, index, _ = walked["pillow_6"]
    with pytest.raises(ValueError, match="index"):
        PackRecord("x.png", stream=s, index=index[:-16])
    with pytest.raises(ValueError, match="transcoded"):
        PackRecord("x.png", stream=s, index=index, transcoded=90)


def test_a_pack_without_png_records_is_the_same_bytes(walked, tmp_path):
    """The writer's JPEG and RAW paths are untouched: the records of before give, byte for
    byte, the file the writer gave before PNG records existed; PNG records in the same pack
    only add their own ranges and move the others."""
    import hashlib
    from monodepth2_amd.pack import KIND_JPEG, KIND_RAW, FramePack, write_pack
    a = str(tmp_path / "plain.pack")
    recs = jpeg_and_raw_records()
    write_pack(a, recs)
    with open(a, "rb") as f:
        blob = f.read()
    assert (len(blob), hashlib.sha256(blob).hexdigest()) == PARENT_PACK
    c = str(tmp_path / "mixed.pack")
    write_pack(c, png_records(walked) + jpeg_and_raw_records())
    fa, fc = FramePack(a), FramePack(c)
    assert fa.png_segment_bytes == 0 and set(fa.records["kind"]) <= {KIND_JPEG, KIND_RAW}
    shift = sum((int(fc.record(r.name)["data_bytes"]) + 15) // 16 * 16 for r in png_records(walked))
    for rec in recs:
        ra, rc = fa.record(rec.name), fc.record(rec.name)
        assert rc["data_offset"] == ra["data_offset"] + shift
        for field in ("kind", "height", "width", "sampling", "data_bytes", "stream_bytes", "quant", "dc", "ac"):
            assert np.array_equal(ra[field], rc[field]), field
        assert np.array_equal(fa.read(rec.name), fc.read(rec.name))
    fa.close()
    fc.close()
