"""Lossless PNG records in a frame pack (pack.build_pack(png_records=True)) and
loader.BatchLoader(pack=...) decoding them from their segment indexes: 8-bit RGB files become
KIND_PNG records and a gray one stays RAW; an epoch from that pack is bit-equal to the epoch
from the tree through PIL and to the epoch from the RAW pack, with and without threads and
with a tail batch; a batch mixes JPEG, PNG and RAW records; a record with a damaged index is
reported by split line, key and bits; png_records with transcode is refused."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import kitti_tree as KT

from test_loader_jpeg_gpu import FRAME_IDS, H, S, W, assert_same, dataset

pytestmark = pytest.mark.gpu

SEG = 1024


def build(root, out, lines=KT.LINES, **kw):
    from monodepth2_amd.pack import FramePack, build_pack
    stats = build_pack(out, root, [lines], png=True, frame_ids=FRAME_IDS, batch=5, threads=2, **kw)
    return FramePack(out), stats


def batches(ds, threads, pack=None, batch=2, **kw):
    from monodepth2_amd.loader import BatchLoader
    ld = BatchLoader(ds, batch, shuffle=False, seed=5, num_workers=threads, pack=pack, **kw)
    try:
        out = list(ld)
        torch.cuda.synchronize()
    finally:
        ld.close()
    return out, ld.pil_fallbacks


GRAY = KT.DRIVES[0][0] + "/image_03/data/0000000001.png"


@pytest.fixture(scope="module")
def png_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_png_pack"))
    KT.write_tree(root, ext=".png")
    gray = os.path.join(root, GRAY)
    Image.open(gray).convert("L").save(gray)          # a file the device decoder does not take
    return root


@pytest.fixture(scope="module")
def png_pack(png_tree, tmp_path_factory):
    fp, stats = build(png_tree, str(tmp_path_factory.mktemp("packs") / "png.pack"), png_records=True,
                      segment_bytes=SEG)
    assert (stats["frames"], stats["png"], stats["raw"], stats["jpeg"], stats["transcoded"]) == (12, 11, 1, 0, 0)
    assert stats["pack_bytes"] == os.path.getsize(fp.path)
    return fp


@pytest.fixture(scope="module")
def raw_pack(png_tree, tmp_path_factory):
    fp, stats = build(png_tree, str(tmp_path_factory.mktemp("packs") / "raw.pack"))
    assert stats["raw"] == 12 and stats["png"] == 0
    return fp


@pytest.fixture(scope="module")
def pil_batches(png_tree):
    """the epoch from the tree through PIL, computed once and never changed"""
    return batches(dataset(png_tree, ext=".png"), 0)[0]


def test_rgb_files_become_png_records_and_a_gray_one_stays_raw(png_tree, png_pack, raw_pack):
    from monodepth2_amd import pack as P, png_ops
    kinds = {name: int(k) for name, k in zip(png_pack.names, png_pack.records["kind"])}
    assert kinds[GRAY] == P.KIND_RAW and all(k == P.KIND_PNG for n, k in kinds.items() if n != GRAY)
    assert png_pack.png_segment_bytes == SEG and png_pack.transcoded == 0
    key = KT.DRIVES[1][0] + "/image_02/data/0000000002.png"
    with open(os.path.join(png_tree, key), "rb") as f:
        s = png_ops.parse_png(f.read())
    got, index = png_pack.png_stream(key)
    assert (got.height, got.width, got.data) == (s.height, s.width, s.data) and png_pack.size(key) == (s.height, s.width)
    assert np.array_equal(index, png_ops.index_png_batch([s], SEG)[0])
    assert int(png_pack.record(key)["data_bytes"]) == (len(s.data) + 15) // 16 * 16 + png_ops.index_nbytes(
        s.height, s.width, SEG)
    print("pack bytes: png records", png_pack.file_bytes, "raw", raw_pack.file_bytes)
    assert png_pack.file_bytes < raw_pack.file_bytes


@pytest.mark.parametrize("threads", [0, 4])
def test_an_epoch_is_bit_equal_to_pil_and_to_the_raw_pack(png_tree, png_pack, raw_pack, pil_batches, threads):
    got, fallbacks = batches(dataset(png_tree, ext=".png"), threads, png_pack)
    assert fallbacks == 0          # a pack's RAW record is read, not decoded: PIL decodes nothing
    assert_same(got, pil_batches)
    assert_same(got, batches(dataset(png_tree, ext=".png"), threads, raw_pack)[0])


def test_tail_batch(png_tree, png_pack, pil_batches):
    got, _ = batches(dataset(png_tree, ext=".png"), 2, png_pack, drop_last=False)
    want, _ = batches(dataset(png_tree, ext=".png"), 2, drop_last=False)
    assert len(got) == 3 and got[-1][("color", 0, 0)].shape[0] == 1
    assert_same(got, want)


def test_a_batch_mixes_jpeg_png_and_raw_records(tmp_path):
    from monodepth2_amd import jpeg_ops, pack as P
    from monodepth2_amd.datasets import KITTIRAWDataset
    root = str(tmp_path / "tree")
    KT.write_tree(root, ext=".jpg")
    prog = os.path.join(root, KT.DRIVES[1][0], "image_02/data", "%010d.jpg" % 1)
    Image.open(prog).convert("RGB").save(prog, "JPEG", quality=92, progressive=True)
    assert jpeg_ops.parse_jpeg(open(prog, "rb").read()) is None
    png_drive = KT.DRIVES[0][0]
    for cam in (2, 3):
        folder = os.path.join(root, png_drive, "image_0{}/data".format(cam))
        for f in sorted(os.listdir(folder)):
            Image.open(os.path.join(folder, f)).convert("RGB").save(os.path.join(folder, f[:-4] + ".png"))
            os.remove(os.path.join(folder, f))

    class Mixed(KITTIRAWDataset):
        def get_image_path(self, folder, frame_index, side):
            p = super().get_image_path(folder, frame_index, side)
            return p[:-4] + ".png" if folder == png_drive else p

    def ds():
        return Mixed(root, KT.LINES, H, W, FRAME_IDS, S, is_train=True, img_ext=".jpg", seed=5)

    paths = {P.frame_key(p, root): p for i in range(len(KT.LINES)) for p in ds().parse(i).paths}
    out = str(tmp_path / "mixed.pack")
    assert P.write_pack(out, P.records_from_files(paths, "cuda", 4, 2, png_records=True, segment_bytes=SEG)) == 12
    fp = P.FramePack(out)
    kinds = {name: int(k) for name, k in zip(fp.names, fp.records["kind"])}
    assert sorted(kinds.values()).count(P.KIND_PNG) == 6 and sorted(kinds.values()).count(P.KIND_RAW) == 1
    assert kinds[P.frame_key(prog, root)] == P.KIND_RAW
    # the first batch (split lines 0 and 1) holds all three kinds
    first = {kinds[P.frame_key(p, root)] for i in (0, 1) for p in ds().parse(i).paths}
    assert first == {P.KIND_JPEG, P.KIND_RAW, P.KIND_PNG}
    want, _ = batches(ds(), 0)
    assert_same(batches(ds(), 0, fp)[0], want)
    assert_same(batches(ds(), 3, fp)[0], want)
    fp.close()


def test_a_damaged_index_is_reported_by_split_line_key_and_bits(png_tree, png_pack, tmp_path):
    from monodepth2_amd.pack import FramePack
    key = KT.DRIVES[1][0] + "/image_02/data/0000000002.png"
    rec = png_pack.record(key)
    data = bytearray(open(png_pack.path, "rb").read())
    start = int(rec["data_offset"]) + (int(rec["stream_bytes"]) + 15) // 16 * 16
    entry = start + 16 + 24 * 3                       # entry 3: its out_pos one too far
    out_pos = int.from_bytes(data[entry + 16:entry + 20], "little")
    data[entry + 16:entry + 20] = (out_pos + 1).to_bytes(4, "little")
    bad = str(tmp_path / "bad.pack")
    with open(bad, "wb") as f:
        f.write(data)
    fp = FramePack(bad)
    for threads in (0, 2):
        with pytest.raises(RuntimeError, match="did not decode") as e:
            batches(dataset(png_tree, ext=".png"), threads, fp)
        text = str(e.value)
        assert "0000000002.png" in text and KT.DRIVES[1][0] in text and "split line 1" in text
        assert "status 64" in text and "segment index" in text
    fp.close()


def test_png_records_with_transcode_is_refused(png_tree, tmp_path):
    with pytest.raises(ValueError, match="png_records and transcode"):
        build(png_tree, str(tmp_path / "no.pack"), png_records=True, transcode=(92, "4:2:0"))
    assert not os.path.exists(str(tmp_path / "no.pack"))


def test_pack_dataset_command_line(png_tree, png_pack, tmp_path, capsys):
    from monodepth2_amd import pack_dataset
    splits = KT.write_splits(str(tmp_path / "splits"))
    out = str(tmp_path / "cli.pack")
    stats = pack_dataset.main(["--data_path", png_tree, "--lists", os.path.join(splits, "train_files.txt"),
                               os.path.join(splits, "val_files.txt"), "--out", out, "--frame_ids", "0", "-1", "1",
                               "--png", "--png_records", "--segment_bytes", str(SEG), "--batch", "5"])
    assert (stats["frames"], stats["png"], stats["raw"]) == (12, 11, 1)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["out"] == out
    with open(out, "rb") as a, open(png_pack.path, "rb") as b:
        assert a.read() == b.read()                   # the same pack as build_pack's
