"""The packed frame file on the host (monodepth2_amd/pack.py): write_pack -> FramePack
round-trips every field, stream byte and index byte of every JPEG case (indexes restated on
the host, tests/jpeg_index_case.py), stores equal tables once, round-trips RAW records,
refuses truncated / foreign / other-version files by name of the problem, names the frame a
dataset lacks, and `--pack` parses.  No GPU."""
import os
import struct

import numpy as np
import pytest

import jpeg_case as jc
import jpeg_index_case as ic
import kitti_tree as KT

from monodepth2_amd import jpeg_ops, pack as P


@pytest.fixture(scope="module")
def records():
    recs = [P.PackRecord("cases/{}.jpg".format(name), stream=jc.parsed(name), index=ic.restated_bytes(name))
            for name in jc.cases()]
    rng = np.random.RandomState(3)
    recs.append(P.PackRecord("raw/odd_7x5.png", raw=rng.randint(0, 256, (7, 5, 3)).astype(np.uint8)))
    recs.append(P.PackRecord("raw/one_1x1.png", raw=rng.randint(0, 256, (1, 1, 3)).astype(np.uint8)))
    return recs


@pytest.fixture(scope="module")
def packed(records, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pack") / "cases.pack")
    assert P.write_pack(path, reversed(records)) == len(records)     # any order in, sorted by name inside
    return path


def test_every_field_stream_byte_and_index_byte_round_trips(records, packed):
    fp = P.FramePack(packed)
    assert len(fp) == len(records) and fp.names == sorted(r.name for r in records)
    assert os.path.getsize(packed) == fp.file_bytes and fp.file_bytes % 16 == 0
    for rec in records:
        if rec.stream is None:
            continue
        s, row = rec.stream, fp.record(rec.name)
        assert rec.name in fp and fp.size(rec.name) == (s.height, s.width)
        assert (row["kind"], row["height"], row["width"], row["sampling"]) == (P.KIND_JPEG, s.height, s.width, s.sampling)
        assert row["stream_bytes"] == len(s.data) and row["data_offset"] % 16 == 0
        assert row["data_bytes"] == (len(s.data) + 15) // 16 * 16 + jpeg_ops.index_nbytes(len(s.data))
        raw = fp.read(rec.name)
        assert raw[:len(s.data)].tobytes() == s.data
        assert not raw[len(s.data):(len(s.data) + 15) // 16 * 16].any()
        assert np.array_equal(raw[(len(s.data) + 15) // 16 * 16:], rec.index)
        for c in range(3):                                            # the tables behind the ids
            assert tuple(fp.quant[row["quant"][c]].view("<u2")) == s.quant[c]
            for cls, ids, own in ((0, row["dc"], s.dc), (1, row["ac"], s.ac)):
                counts, vals = s.huff[(cls, own[c])]
                t = fp.huff[ids[c]]
                assert tuple(t[:16]) == counts and t[16:16 + len(vals)].tobytes() == vals and not t[16 + len(vals):].any()
        got, index = fp.stream(rec.name)                             # and as the decoder takes them
        assert (got.height, got.width, got.sampling, got.factors, got.data) == (s.height, s.width, s.sampling,
                                                                              s.factors, s.data)
        assert got.quant == s.quant and np.array_equal(index, rec.index)
        assert [got.huff[(0, t)] for t in got.dc] == [s.huff[(0, t)] for t in s.dc]
        assert [got.huff[(1, t)] for t in got.ac] == [s.huff[(1, t)] for t in s.ac]
        states, first = jpeg_ops.unpack_index(index, len(s.data))
        want = ic.restated(rec.name[len("cases/"):-len(".jpg")])
        assert states.tolist() == want[0] and first.tolist() == want[1]
    fp.close()


def test_equal_tables_are_stored_once(records, packed):
    fp = P.FramePack(packed)
    streams = [r.stream for r in records if r.stream is not None]
    quant = {s.quant[c] for s in streams for c in range(3)}
    huff = {s.huff[(cls, t)] for s in streams for cls, ids in ((0, s.dc), (1, s.ac)) for t in ids}
    assert len(fp.quant) == len(quant) and len(fp.huff) == len(huff)
    assert len({t.tobytes() for t in fp.quant}) == len(quant) and len({t.tobytes() for t in fp.huff}) == len(huff)
    # the unoptimised cases share the standard tables, the optimised ones carry their own
    assert len(huff) < 4 * len(streams) and len(huff) > 4
    plain = [fp.record("cases/{}.jpg".format(n)) for n in jc.cases() if not n.endswith("_opt")]
    assert len({tuple(r["dc"]) + tuple(r["ac"]) for r in plain}) == 1
    fp.close()


def test_a_raw_record_round_trips(records, packed):
    fp = P.FramePack(packed)
    for rec in records:
        if rec.raw is None:
            continue
        row = fp.record(rec.name)
        h, w = rec.raw.shape[:2]
        assert (row["kind"], row["height"], row["width"], row["data_bytes"]) == (P.KIND_RAW, h, w, h * w * 3)
        assert fp.size(rec.name) == (h, w) and np.array_equal(fp.read(rec.name).reshape(h, w, 3), rec.raw)
        with pytest.raises(ValueError, match="RAW"):
            fp.stream(rec.name)
    with pytest.raises(KeyError, match="not in the pack"):
        fp.record("cases/absent.jpg")
    fp.close()


def test_records_must_be_whole(records):
    s = records[0].stream
    with pytest.raises(ValueError, match="index of"):
        P.PackRecord("x", stream=s, index=np.zeros(4, np.uint8))
    with pytest.raises(ValueError, match="either"):
        P.PackRecord("x")
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        P.PackRecord("x", raw=np.zeros((4, 4), np.uint8))


def test_a_name_twice_is_refused(records, tmp_path):
    with pytest.raises(ValueError, match="twice"):
        P.write_pack(str(tmp_path / "twice.pack"), [records[0], records[0]])


def test_truncated_foreign_and_other_version_files_are_refused(packed, tmp_path):
    data = open(packed, "rb").read()

    def refused(name, content, match):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(content)
        with pytest.raises(P.PackError, match=match):
            P.FramePack(path)

    refused("cut_tail.pack", data[:-16], "truncated")
    refused("cut_half.pack", data[:len(data) // 2], "truncated")
    refused("cut_header.pack", data[:40], "truncated")
    refused("empty.pack", b"", "truncated")
    refused("magic.pack", b"MD2PACX\0" + data[8:], "wrong magic")
    refused("unfinished.pack", b"\0" * P.HEADER_BYTES + data[P.HEADER_BYTES:], "wrong magic")
    refused("version.pack", data[:8] + struct.pack("<I", P.VERSION + 1) + data[12:], "wrong version 2")
    # a record that points past the data is a damaged file too
    fp = P.FramePack(packed)
    rec_off = struct.unpack_from("<Q", data, 56)[0]
    fp.close()
    bad = bytearray(data)
    struct.pack_into("<Q", bad, rec_off + 24, len(data))            # record 0's data_bytes
    refused("record.pack", bytes(bad), "outside")


def test_covers_names_a_missing_frame_by_split_line_and_path(tmp_path):
    from monodepth2_amd.datasets import KITTIRAWDataset
    root = str(tmp_path / "tree")
    rng = np.random.RandomState(5)

    def ds(lines, frame_ids=(0, -1, 1)):
        return KITTIRAWDataset(root, lines, 64, 128, list(frame_ids), 4, is_train=True, img_ext=".jpg")

    # records named as build_pack names them, for lines 0 and 1 only (the left camera)
    full = ds(KT.LINES)
    keys = sorted({P.frame_key(p, root) for i in (0, 1) for p in full.parse(i).paths})
    assert keys[0] == KT.DRIVES[0][0] + "/image_02/data/0000000000.jpg" and len(keys) == 6
    path = str(tmp_path / "left.pack")
    P.write_pack(path, [P.PackRecord(k, raw=rng.randint(0, 256, (3, 4, 3)).astype(np.uint8)) for k in keys])
    fp = P.FramePack(path)
    assert fp.covers(ds(KT.LINES[:2])) and fp.missing(ds(KT.LINES[:2])) is None
    assert fp.covers(ds(KT.LINES[:2], [0]))
    assert not fp.covers(full)
    msg = fp.missing(full)
    assert "split line 2" in msg and KT.LINES[2] in msg
    assert os.path.join(root, KT.DRIVES[0][0], "image_03/data", "0000000001.jpg") in msg and path in msg
    assert "image_03/data/0000000000.jpg" not in msg                  # the first frame it lacks, in frame id order
    fp.close()


def test_frame_key_is_relative_with_forward_slashes():
    assert P.frame_key("/data/kitti/a/b/0000000001.jpg", "/data/kitti") == "a/b/0000000001.jpg"
    assert P.frame_key("/data/kitti/a/b.jpg", "/data/kitti/") == "a/b.jpg"
    assert P.frame_key("/data/other/a.jpg", "/data/kitti") == "../other/a.jpg"


def test_pack_flag_parses():
    from monodepth2_amd.options import MonodepthOptions
    from monodepth2_amd.pack import open_pack
    opt = MonodepthOptions().parse([])
    assert opt.pack is None and open_pack(opt) is None
    opt = MonodepthOptions().parse(["--pack", "/some/where/kitti.pack", "--num_workers", "4"])
    assert opt.pack == "/some/where/kitti.pack" and not opt.device_decode


def test_index_helpers():
    assert [jpeg_ops.index_nsub(b) for b in (0, 1, 128, 129, 256, 257)] == [1, 1, 1, 2, 2, 3]
    assert [jpeg_ops.index_nbytes(b) for b in (0, 128, 129, 257, 4 * 128)] == [16, 16, 32, 48, 48]
    idx = jpeg_ops.pack_index([0, (1030 << 16) | (2 << 8) | 5, 2048 << 16], [0, 7, 9])
    assert idx.dtype == np.uint8 and idx.size == 48 and not idx[36:].any()
    states, first = jpeg_ops.unpack_index(idx, 300)
    assert states.tolist() == [0, (1030 << 16) | (2 << 8) | 5, 2048 << 16] and first.tolist() == [0, 7, 9]
    with pytest.raises(ValueError):
        jpeg_ops.unpack_index(idx, 100)
    with pytest.raises(ValueError):
        jpeg_ops.pack_index([0, 1], [0])
