"""loader.BatchLoader(pack=FramePack) against the PIL path on JPEG trees (tests/kitti_tree.py)
packed with pack.build_pack, mirroring test_loader_jpeg_gpu.py: every tensor of every batch
bit-equal with and without threads, with a tail batch, at 4:2:0 and 4:2:2; the packed loader
runs with the image files gone; PNG and progressive files pack as RAW and stay bit-equal; a
pack that lacks a line's frame refuses the loader at construction; a damaged index is
reported by split line and frame; `train --pack` logs the losses of the run without it."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import kitti_tree as KT

from test_loader_jpeg_gpu import FRAME_IDS, H, S, W, assert_same, dataset, resave

pytestmark = pytest.mark.gpu


def build(root, out, lines=KT.LINES, **kw):
    from monodepth2_amd.pack import FramePack, build_pack
    stats = build_pack(out, root, [lines], frame_ids=FRAME_IDS, batch=5, threads=2, **kw)   # several device calls
    return FramePack(out), stats


def batches(ds, threads, pack=None, batch=2, **kw):
    from monodepth2_amd.loader import BatchLoader
    ld = BatchLoader(ds, batch, shuffle=False, seed=5, num_workers=threads, pack=pack, **kw)
    try:
        out = list(ld)
        torch.cuda.synchronize()
    finally:
        ld.close()
    return out


@pytest.fixture(scope="module")
def tree420(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti420"))
    KT.write_tree(root, ext=".jpg")
    return root


@pytest.fixture(scope="module")
def tree422(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti422"))
    KT.write_tree(root, ext=".jpg", seed=1)
    resave(root, 1)
    return root


@pytest.fixture(scope="module")
def pack420(tree420, tmp_path_factory):
    fp, stats = build(tree420, str(tmp_path_factory.mktemp("packs") / "420.pack"))
    assert stats["frames"] == stats["jpeg"] == 12 == len(fp) and stats["raw"] == 0
    assert stats["pack_bytes"] == os.path.getsize(fp.path) and stats["file_bytes"] > 0
    return fp


@pytest.fixture(scope="module")
def pack422(tree422, tmp_path_factory):
    fp, _ = build(tree422, str(tmp_path_factory.mktemp("packs") / "422.pack"))
    assert {int(s) for s in fp.records["sampling"]} == {1}
    return fp


@pytest.fixture(scope="module")
def pil420(tree420):
    return batches(dataset(tree420), 0)


@pytest.mark.parametrize("threads", [0, 4])
def test_packed_batches_are_bit_equal_to_pil(tree420, tree422, pack420, pack422, pil420, threads):
    assert_same(batches(dataset(tree420), threads, pack420), pil420)
    assert_same(batches(dataset(tree422), threads, pack422), batches(dataset(tree422), threads))


def test_the_pack_keys_frames_by_relative_path_and_keeps_stream_and_index_together(tree420, pack420):
    from monodepth2_amd import jpeg_ops
    key = KT.DRIVES[1][0] + "/image_03/data/0000000002.jpg"
    assert key in pack420 and pack420.size(key) == KT.DRIVES[1][1]
    with open(os.path.join(tree420, key), "rb") as f:
        s = jpeg_ops.parse_jpeg(f.read())
    got, index = pack420.stream(key)
    assert got.data == s.data and got.quant == s.quant
    assert np.array_equal(index, jpeg_ops.index_jpeg_batch([s], "cuda")[0])


def test_tail_batch(tree420, pack420):
    got = batches(dataset(tree420), 2, pack420, drop_last=False)
    want = batches(dataset(tree420), 2, drop_last=False)
    assert len(got) == 3 and got[-1][("color", 0, 0)].shape[0] == 1
    assert_same(got, want)


def test_the_packed_loader_runs_with_the_image_files_gone(tmp_path):
    root = str(tmp_path / "tree")
    KT.write_tree(root, ext=".jpg")
    want = batches(dataset(root), 2)
    fp, _ = build(root, str(tmp_path / "tree.pack"))
    for drive, _ in KT.DRIVES:
        shutil.rmtree(os.path.join(root, drive))
    with pytest.raises(FileNotFoundError):
        batches(dataset(root), 2)
    assert_same(batches(dataset(root), 2, fp), want)
    assert_same(batches(dataset(root), 0, fp), want)
    fp.close()


def test_png_and_progressive_files_pack_as_raw_and_stay_bit_equal(tmp_path):
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

    # build_pack names frames through the dataset classes; the mixed tree goes in as records
    paths = {P.frame_key(p, root): p for i in range(len(KT.LINES)) for p in ds().parse(i).paths}
    out = str(tmp_path / "mixed.pack")
    assert P.write_pack(out, P.records_from_files(paths, "cuda", 4, 2)) == 12
    fp = P.FramePack(out)
    kinds = {name: int(k) for name, k in zip(fp.names, fp.records["kind"])}
    assert sum(k == P.KIND_RAW for k in kinds.values()) == 6 + 1
    assert kinds[P.frame_key(prog, root)] == P.KIND_RAW and all(k == P.KIND_RAW for n, k in kinds.items() if n.endswith(".png"))
    assert fp.covers(ds())
    want = batches(ds(), 0)
    assert_same(batches(ds(), 0, fp), want)
    assert_same(batches(ds(), 3, fp), want)
    fp.close()


def test_a_png_tree_packs_with_the_png_flag(tmp_path):
    root = str(tmp_path / "tree")
    KT.write_tree(root, ext=".png")
    fp, stats = build(root, str(tmp_path / "png.pack"), png=True)
    assert stats["raw"] == 12 and stats["jpeg"] == 0
    assert_same(batches(dataset(root, ext=".png"), 2, fp), batches(dataset(root, ext=".png"), 2))
    fp.close()


def test_a_pack_of_other_lines_refuses_the_loader_at_construction(tree420, tmp_path):
    from monodepth2_amd.loader import BatchLoader
    fp, stats = build(tree420, str(tmp_path / "left.pack"), lines=KT.LINES[:2])      # the left camera only
    assert stats["frames"] == 6
    assert_same(batches(dataset(tree420, KT.LINES[:2]), 0, fp), batches(dataset(tree420, KT.LINES[:2]), 0))
    with pytest.raises(ValueError, match="is not in the pack") as e:
        BatchLoader(dataset(tree420), 2, shuffle=False, pack=fp)
    assert "split line 2" in str(e.value) and KT.LINES[2] in str(e.value) and "image_03/data/0000000001.jpg" in str(e.value)
    fp.close()
    with pytest.raises(FileNotFoundError, match="no such image file"):
        build(tree420, str(tmp_path / "absent.pack"), lines=["{} 5 l".format(KT.DRIVES[0][0])])
    assert not os.path.exists(str(tmp_path / "absent.pack")) and not os.path.exists(str(tmp_path / "absent.pack.tmp"))


def test_a_damaged_index_is_reported_by_split_line_and_frame(tree420, pack420, tmp_path):
    from monodepth2_amd.pack import FramePack
    key = KT.DRIVES[1][0] + "/image_02/data/0000000002.jpg"
    rec = pack420.record(key)
    data = bytearray(open(pack420.path, "rb").read())
    start = int(rec["data_offset"]) + (int(rec["stream_bytes"]) + 15) // 16 * 16
    data[start + 8:int(rec["data_offset"]) + int(rec["data_bytes"])] = bytes(
        int(rec["data_offset"]) + int(rec["data_bytes"]) - start - 8)              # all but the first state zeroed
    bad = str(tmp_path / "bad.pack")
    with open(bad, "wb") as f:
        f.write(data)
    fp = FramePack(bad)
    for threads in (0, 2):
        with pytest.raises(RuntimeError, match="did not decode") as e:
            batches(dataset(tree420), threads, fp)
        assert "0000000002.jpg" in str(e.value) and KT.DRIVES[1][0] in str(e.value) and "split line 1" in str(e.value)
        assert "index" in str(e.value)
    fp.close()


def test_pack_dataset_command_line(tree420, tmp_path, capsys):
    from monodepth2_amd import pack_dataset
    from monodepth2_amd.pack import FramePack
    splits = KT.write_splits(str(tmp_path / "splits"))
    out = str(tmp_path / "cli.pack")
    stats = pack_dataset.main(["--data_path", tree420, "--lists", os.path.join(splits, "train_files.txt"),
                               os.path.join(splits, "val_files.txt"), "--out", out, "--frame_ids", "0", "-1", "1"])
    assert stats["frames"] == 12 and json.loads(capsys.readouterr().out.strip().splitlines()[-1])["out"] == out
    fp = FramePack(out)
    assert fp.covers(dataset(tree420))
    fp.close()


def test_train_cli_logs_the_same_losses_with_a_pack(tmp_path):
    from monodepth2_amd import train
    root = str(tmp_path / "tree")
    KT.write_tree(root, ext=".jpg")
    KT.write_velodyne(root)
    splits = KT.write_splits(os.path.join(root, "splits"))
    fp, _ = build(root, str(tmp_path / "train.pack"))
    fp.close()

    def run(name, *extra):
        torch.manual_seed(11)   # --weights_init scratch draws the networks from the global generator
        tr = train.main(["--data_path", root, "--split_dir", splits, "--log_dir", str(tmp_path),
                         "--model_name", name, "--height", "64", "--width", "128", "--batch_size", "2",
                         "--num_epochs", "1", "--log_frequency", "1", "--weights_init", "scratch", "--num_workers", "2",
                         *extra])
        assert tr.step == 2
        with open(tmp_path / name / "train" / "scalars.jsonl") as f:
            return [json.loads(line) for line in f]

    a, b = run("pil"), run("packed", "--pack", str(tmp_path / "train.pack"))
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        for k in ["loss"] + ["loss/{}".format(s) for s in range(4)]:
            assert x[k] == y[k], (k, x[k], y[k])
