"""monodepth2_amd.datasets: the reference's split-line rules and paths (held to a golden
recorded from the reference's own classes, tests/golden/dataset/make_dataset_golden.py)
and the decoding contract (native size, RGB, unflipped) on a tiny tree written with PIL."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from PIL import Image

import kitti_tree as KT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset", "dataset_paths.json")
ROOT = "/data/kitti"


def _cases():
    with open(GOLDEN) as f:
        return json.load(f)


def test_paths_sides_and_stereo_sign_match_the_reference():
    from monodepth2_amd import datasets as D
    from monodepth2_amd.augment import stereo_tx
    cases = _cases()
    assert sum(len(c["items"]) for c in cases) >= 12
    seen = set()
    for c in cases:
        cls = getattr(D, c["dataset"])
        lines = [it["line"] for it in c["items"]]
        ds = cls(ROOT, lines, 192, 640, c["frame_idxs"], 4, is_train=c["is_train"], img_ext=c["img_ext"])
        assert np.array_equal(ds.K, np.array(c["K"], np.float32)) and ds.K.dtype == np.float32
        assert list(ds.full_res_shape) == c["full_res_shape"] and ds.side_map == c["side_map"]
        for i, want in enumerate(c["items"]):
            if "error" in want:     # a one-field line: frame 0 and no side, which side_map cannot index
                with pytest.raises(KeyError):
                    ds.parse(i)
                assert want["error"] == "KeyError"
                seen.add("one-field")
                continue
            item = ds.parse(i)
            assert [os.path.relpath(p, ROOT) for p in item.paths] == want["paths"], want["line"]
            assert item.side == want["sides"][0]
            if "s" in c["frame_idxs"]:
                k = c["frame_idxs"].index("s")
                assert want["sides"][k] == {"l": "r", "r": "l"}[item.side]
                assert np.float32(stereo_tx(item.side, want["do_flip"])) == np.float32(want["stereo_tx"])
                seen.add("stereo flip" if want["do_flip"] else "stereo")
            seen.add(c["dataset"] + item.side)
            if not c["is_train"]:
                assert not item.draw.do_flip and not item.draw.do_color_aug
    assert {"one-field", "stereo", "stereo flip", "KITTIRAWDatasetl", "KITTIRAWDatasetr", "KITTIOdomDatasetl",
            "KITTIDepthDatasetr"} <= seen


def test_readlines(tmp_path):
    from monodepth2_amd.datasets import readlines
    p = tmp_path / "x.txt"
    p.write_text("a 1 l\nb 2 r\n")
    assert readlines(str(p)) == ["a 1 l", "b 2 r"]


@pytest.mark.parametrize("ext", [".png", ".jpg"])
def test_frames_are_the_decoded_files_unflipped(tmp_path, ext):
    from monodepth2_amd.datasets import KITTIRAWDataset
    written = KT.write_tree(str(tmp_path), ext=ext)
    ds = KITTIRAWDataset(str(tmp_path), KT.LINES, 64, 128, [0, -1, 1, "s"], 4, is_train=True, img_ext=ext, seed=3)
    flips = 0
    for i, line in enumerate(KT.LINES):
        item = ds[i]
        drive, _, side = line.split()
        assert item.side == side and item.size == dict(KT.DRIVES)[drive]
        cams = [{"l": 2, "r": 3}[side]] * 3 + [{"l": 3, "r": 2}[side]]
        for arr, frame, cam in zip(item.frames, (1, 0, 2, 1), cams):
            rel = os.path.join(drive, "image_0{}/data".format(cam), "{:010d}{}".format(frame, ext))
            want = np.asarray(Image.open(os.path.join(str(tmp_path), rel)).convert("RGB"))
            assert arr.dtype == np.uint8 and arr.shape == item.size + (3,)
            assert np.array_equal(arr, want), rel      # never flipped, whatever the draw says
            if ext == ".png":
                assert np.array_equal(arr, written[rel])
        flips += item.draw.do_flip
    assert 0 < flips < len(KT.LINES)    # the draws do ask for flips; the frames above ignore them


def test_check_depth_and_depth_dataset(tmp_path):
    from monodepth2_amd.datasets import KITTIDepthDataset, KITTIRAWDataset
    KT.write_tree(str(tmp_path / "plain"))
    KT.write_tree(str(tmp_path / "gt"), depth=True)
    args = (KT.LINES, 64, 128, [0, -1, 1], 4)
    assert not KITTIRAWDataset(str(tmp_path / "plain"), *args, img_ext=".png").check_depth()
    assert not KITTIRAWDataset(str(tmp_path / "plain"), *args, img_ext=".png", load_depth=True).load_depth
    assert KITTIRAWDataset(str(tmp_path / "gt"), *args, img_ext=".png").check_depth()
    ds = KITTIDepthDataset(str(tmp_path / "gt"), *args, img_ext=".png", load_depth=True)
    assert ds.load_depth
    assert not KITTIDepthDataset(str(tmp_path / "gt"), *args, img_ext=".png").load_depth   # only when asked for
    for line in KT.LINES[:4]:
        drive, frame, side = line.split()
        path = os.path.join(str(tmp_path / "gt"), drive, "proj_depth/groundtruth/image_0{}".format(ds.side_map[side]),
                            "{:010d}.png".format(int(frame)))
        # the reference's three lines (kitti_dataset.py:127-129), then its flip
        want = Image.open(path)
        want = want.resize((1242, 375), Image.NEAREST)
        want = np.array(want).astype(np.float32) / 256
        got = ds.get_depth(drive, int(frame), side, False)
        assert got.shape == (375, 1242) and got.dtype == np.float32 and np.array_equal(got, want)
        assert want.max() > 1 and (want == 0).any()
        assert np.array_equal(ds.get_depth(drive, int(frame), side, True), np.fliplr(want))


@pytest.mark.parametrize("n_in,n_out", [(370, 375), (374, 375), (376, 375), (1226, 1242), (1238, 1242),
                                        (1241, 1242), (375, 375), (7, 3)])
def test_nearest_index_is_pils_rule(n_in, n_out):
    """KITTIRAWDataset.get_depth resamples the other three KITTI sizes with this gather."""
    from monodepth2_amd.datasets import nearest_index
    ramp = np.arange(n_in, dtype=np.int32)
    cols = np.array(Image.fromarray(np.tile(ramp, (2, 1))).resize((n_out, 2), Image.NEAREST))[0]
    rows = np.array(Image.fromarray(np.tile(ramp[:, None], (1, 2))).resize((2, n_out), Image.NEAREST))[:, 0]
    idx = nearest_index(n_in, n_out)
    assert np.array_equal(idx, cols) and np.array_equal(idx, rows)


def test_missing_file_names_the_line(tmp_path):
    from monodepth2_amd.datasets import KITTIRAWDataset
    KT.write_tree(str(tmp_path))
    lines = KT.LINES[:1] + ["{} 2 l".format(KT.DRIVES[1][0])]     # frame 3 does not exist
    ds = KITTIRAWDataset(str(tmp_path), lines, 64, 128, [0, -1, 1], 4, img_ext=".png")
    ds[0]
    with pytest.raises(FileNotFoundError) as e:
        ds[1]
    assert lines[1] in str(e.value) and "0000000003.png" in str(e.value) and "line 1" in str(e.value)


def test_frames_of_one_item_must_agree_in_size(tmp_path):
    from monodepth2_amd.datasets import KITTIRAWDataset
    KT.write_tree(str(tmp_path))
    drive = KT.DRIVES[0][0]
    Image.new("RGB", (50, 40)).save(os.path.join(str(tmp_path), drive, "image_02/data/0000000002.png"))
    ds = KITTIRAWDataset(str(tmp_path), KT.LINES, 64, 128, [0, -1, 1], 4, img_ext=".png")
    with pytest.raises(ValueError, match="different sizes"):
        ds[0]


def test_draws_depend_on_seed_epoch_index_only(tmp_path):
    from monodepth2_amd.augment import draw_item
    from monodepth2_amd.datasets import KITTIRAWDataset, item_seed
    import random
    KT.write_tree(str(tmp_path))
    lines = KT.LINES * 4
    ds = KITTIRAWDataset(str(tmp_path), lines, 64, 128, [0, -1, 1], 4, is_train=True, img_ext=".png", seed=11)
    serial = [ds.parse(i, epoch=2).draw for i in range(len(lines))]
    for threads in (1, 4):
        with ThreadPoolExecutor(threads) as pool:
            got = list(pool.map(lambda i: ds.open_item(i, 2).draw, reversed(range(len(lines)))))[::-1]
        assert got == serial
    assert serial == [draw_item(random.Random(item_seed(11, 2, i))) for i in range(len(lines))]
    assert serial != [ds.parse(i, epoch=3).draw for i in range(len(lines))]
    ds.set_epoch(2)
    assert [ds[i].draw for i in range(4)] == serial[:4]
    assert any(d.do_color_aug for d in serial) and any(not d.do_color_aug for d in serial)
