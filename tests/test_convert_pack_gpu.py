"""`convert_dataset` and transcoded packs on a synthetic KITTI tree of PNGs (tests/kitti_tree.py:
two frame sizes, twelve frames): the converted files are Pillow's, byte for byte; a pack built
with transcode holds only JPEG records, the unstuffed Pillow bodies under the .png keys, and is
smaller; and a batch from it is bit-equal to the batch from the converted tree read as .jpg
with device_decode."""
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import kitti_tree as KT

from test_loader_jpeg_gpu import FRAME_IDS, assert_same, dataset

pytestmark = pytest.mark.gpu

QUALITY, SUBSAMPLING = 92, 2      # the reference's convert -quality 92 -sampling-factor 2x2,1x1,1x1


def pillow_jpeg(png_path, quality=QUALITY, subsampling=SUBSAMPLING) -> bytes:
    buf = io.BytesIO()
    Image.open(png_path).convert("RGB").save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def pngs_of(root):
    return sorted(os.path.join(d, f) for d, _, files in os.walk(root) for f in files if f.endswith(".png"))


def batches(ds, threads, pack=None, device_decode=False):
    from monodepth2_amd.loader import BatchLoader
    ld = BatchLoader(ds, 2, shuffle=False, seed=5, num_workers=threads, pack=pack, device_decode=device_decode)
    try:
        out = list(ld)
        torch.cuda.synchronize()
    finally:
        ld.close()
    return out


@pytest.fixture(scope="module")
def png_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_png"))
    KT.write_tree(root, ext=".png")
    pngs = pngs_of(root)
    assert len(pngs) == 12 and len({Image.open(p).size for p in pngs}) == 2
    return root


@pytest.fixture(scope="module")
def want(png_tree):
    """png path -> Pillow's file, computed once and never changed"""
    return {p: pillow_jpeg(p) for p in pngs_of(png_tree)}


@pytest.fixture(scope="module")
def converted(png_tree, want):
    """the tree after `convert_dataset` (the PNGs kept)"""
    from monodepth2_amd import convert_dataset
    stats = convert_dataset.main(["--data_path", png_tree, "--batch", "5", "--threads", "3"])
    assert stats["frames"] == stats["converted"] == 12 and stats["skipped"] == stats["removed"] == 0
    assert stats["bytes_in"] == sum(os.path.getsize(p) for p in want)
    assert stats["bytes_out"] == sum(len(b) for b in want.values())
    return png_tree


def test_converted_files_are_pillows(converted, want, capsys):
    from monodepth2_amd import convert_dataset
    for p, ref in want.items():
        assert os.path.exists(p)                                   # kept without --remove_png
        with open(p[:-4] + ".jpg", "rb") as f:
            assert f.read() == ref, p
    assert not [f for d, _, files in os.walk(converted) for f in files if f.endswith(".tmp")]
    before = {p: os.stat(p[:-4] + ".jpg").st_mtime_ns for p in want}
    stats = convert_dataset.main(["--data_path", converted])      # a second run skips
    assert stats["skipped"] == 12 and stats["converted"] == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["skipped"] == 12
    assert before == {p: os.stat(p[:-4] + ".jpg").st_mtime_ns for p in want}


def test_lists_quality_sampling_and_remove_png(tmp_path):
    """--lists converts the frames the lines name; --remove_png removes only converted files"""
    from monodepth2_amd import convert_dataset
    root = str(tmp_path / "tree")
    KT.write_tree(root, ext=".png")
    splits = str(tmp_path / "splits")
    KT.write_splits(splits, train=KT.LINES[:1], val=KT.LINES[:1])   # drive 0, left camera, frames 0..2
    named = [os.path.join(root, KT.DRIVES[0][0], "image_02/data", "%010d.png" % i) for i in range(3)]
    ref = {p: pillow_jpeg(p, 75, 1) for p in named}
    kept = named[0][:-4] + ".jpg"
    with open(kept, "wb") as f:
        f.write(b"already here")
    stats = convert_dataset.main(["--data_path", root, "--lists", os.path.join(splits, "train_files.txt"),
                                  "--quality", "75", "--sampling", "422", "--remove_png"])
    assert (stats["frames"], stats["converted"], stats["skipped"], stats["removed"]) == (3, 2, 1, 2)
    assert open(kept, "rb").read() == b"already here" and os.path.exists(named[0])   # skipped: its PNG stays
    for p in named[1:]:
        assert not os.path.exists(p) and open(p[:-4] + ".jpg", "rb").read() == ref[p]
    assert len(pngs_of(root)) == 12 - 2
    stats = convert_dataset.main(["--data_path", root, "--quality", "75", "--sampling", "422", "--overwrite"])
    assert (stats["frames"], stats["converted"], stats["skipped"]) == (10, 10, 0)     # every PNG still there
    assert open(kept, "rb").read() == ref[named[0]]


@pytest.fixture(scope="module")
def packs(png_tree, tmp_path_factory):
    from monodepth2_amd.pack import FramePack, build_pack
    folder = tmp_path_factory.mktemp("packs")
    out = {}
    for name, kw in (("raw", {}), ("transcoded", {"transcode": (QUALITY, "4:2:0")})):
        path = str(folder / (name + ".pack"))
        stats = build_pack(path, png_tree, [KT.LINES], png=True, frame_ids=FRAME_IDS, batch=5, threads=2, **kw)
        out[name] = (FramePack(path), stats)
    return out


def test_transcoded_pack_holds_pillows_streams(packs, want, png_tree):
    from monodepth2_amd import jpeg_ops, pack as P
    (raw, raw_stats), (fp, stats) = packs["raw"], packs["transcoded"]
    assert raw_stats["raw"] == 12 and raw_stats["transcoded"] == 0 and raw.transcoded == 0
    assert stats["frames"] == stats["jpeg"] == stats["transcoded"] == 12 and stats["raw"] == 0
    assert (fp.records["kind"] == P.KIND_JPEG).all() and fp.transcoded == 12
    assert (fp.records["reserved"][:, 0] == 1).all() and (fp.records["reserved"][:, 1] == QUALITY).all()
    assert (fp.records["reserved"][:, 2:] == 0).all() and (raw.records["reserved"] == 0).all()
    print("pack bytes: raw", raw_stats["pack_bytes"], "transcoded", stats["pack_bytes"])
    assert stats["pack_bytes"] < raw_stats["pack_bytes"]
    assert sorted(fp.names) == sorted(raw.names) and all(n.endswith(".png") for n in fp.names)
    for p, ref in want.items():
        key = P.frame_key(p, png_tree)
        s, index = fp.stream(key)
        r = jpeg_ops.parse_jpeg(ref)
        assert s.data == r.data and s.quant == r.quant and (s.height, s.width, s.sampling) == (r.height, r.width, 2)
        assert jpeg_ops.jpeg_file_bytes(s) == ref
        assert index.size == jpeg_ops.index_nbytes(len(s.data))


@pytest.mark.parametrize("threads", [0, 3])
def test_transcoded_pack_batches_equal_the_converted_tree(packs, converted, threads):
    got = batches(dataset(converted, ext=".png"), threads, pack=packs["transcoded"][0])
    assert_same(got, batches(dataset(converted, ext=".jpg"), threads, device_decode=True))
    assert_same(got, batches(dataset(converted, ext=".jpg"), 0))        # and so Pillow's decode of those files


def test_pack_dataset_transcode_flag_and_the_training_notice(png_tree, tmp_path, capsys):
    from types import SimpleNamespace
    from monodepth2_amd import pack as P, pack_dataset
    splits = str(tmp_path / "splits")
    KT.write_splits(splits)
    out = str(tmp_path / "cli.pack")
    stats = pack_dataset.main(["--data_path", png_tree, "--lists", os.path.join(splits, "train_files.txt"), "--out", out,
                               "--png", "--transcode", "--quality", "75", "--sampling", "444"])
    assert stats["transcoded"] == stats["frames"] == 12
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["transcoded"] == 12
    fp = P.open_pack(SimpleNamespace(pack=out))
    text = capsys.readouterr().out
    assert text.count("\n") == 1 and "lossy" in text and "quality 75" in text
    assert {int(s) for s in fp.records["sampling"]} == {0}
    fp.close()
    plain = str(tmp_path / "plain.pack")
    pack_dataset.main(["--data_path", png_tree, "--lists", os.path.join(splits, "train_files.txt"), "--out", plain,
                       "--png"])
    capsys.readouterr()
    P.open_pack(SimpleNamespace(pack=plain)).close()
    assert capsys.readouterr().out == ""
