"""loader.BatchLoader on a tiny KITTI-shaped tree (tests/kitti_tree.py): two drives with
native sizes 123 x 243 and 121 x 240, so a batch of 2 mixes two decoded sizes; the feed
is 64 x 128.  Every colour key is held bit-equal to the PIL-pinned oracle on the decoded
files with that item's draw."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import kitti_tree as KT
from oracle import augment_oracle as A

pytestmark = pytest.mark.gpu

H, W, S = 64, 128, 4
FRAME_IDS = [0, -1, 1]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti"))
    KT.write_tree(root, depth=True)
    return root


def _dataset(root, frame_ids=FRAME_IDS, cls=None, **kw):
    from monodepth2_amd.datasets import KITTIRAWDataset
    return (cls or KITTIRAWDataset)(root, KT.LINES, H, W, frame_ids, S, is_train=True, img_ext=".png", seed=5, **kw)


def _loader(ds, threads, **kw):
    from monodepth2_amd.loader import BatchLoader
    kw.setdefault("shuffle", False)
    return BatchLoader(ds, 2, seed=5, num_workers=threads, **kw)


def test_batches_match_the_oracle_with_and_without_threads(tree):
    from monodepth2_amd.data import pack_rgbx, scaled_intrinsics
    ds = _dataset(tree)
    a, b = _loader(ds, 0), _loader(ds, 2)
    got0, got2 = list(a), list(b)
    torch.cuda.synchronize()
    a.close(), b.close()
    assert len(got0) == len(got2) == len(a) == 2      # five lines, batch 2: the partial batch is dropped
    assert a.epoch == 1                               # an exhausted epoch advances it
    for x, y in zip(got0, got2):
        assert x.keys() == y.keys()
        for k in x:
            assert torch.equal(x[k], y[k]), k
    assert a.aug.sizes == [(123, 243), (121, 240)]    # both sizes in one batch, one plan
    for n, batch in enumerate(got0):
        assert "stereo_T" not in batch and "depth_gt" not in batch
        for j, idx in enumerate(a.batches(0)[n]):
            item = ds.parse(idx, epoch=0)
            d = item.draw
            jit = (d.order, d.brightness, d.contrast, d.saturation, d.hue) if d.do_color_aug else None
            for fid, path in zip(FRAME_IDS, item.paths):
                img = np.asarray(Image.open(path).convert("RGB"))
                color, caug = A.preprocess(img, H, W, S, flip=d.do_flip, jitter=jit)
                for s in range(S):
                    assert np.array_equal(batch[("color", fid, s)][j].cpu().numpy(), color[s]), (n, j, fid, s)
                    assert np.array_equal(batch[("color_aug", fid, s)][j].cpu().numpy(), caug[s]), (n, j, fid, s)
        assert torch.equal(batch["color_src8"], pack_rgbx([batch[("color", f, 0)] for f in FRAME_IDS[1:]]))
        for s in range(S):
            K, inv_K = scaled_intrinsics(H, W, s)
            assert np.array_equal(batch[("K", s)].cpu().numpy(), np.tile(K, (2, 1, 1)))
            assert np.array_equal(batch[("inv_K", s)].cpu().numpy(), np.tile(inv_K, (2, 1, 1)))


def test_shuffle_epochs_and_rank_shards(tree):
    ds = _dataset(tree)
    whole = _loader(ds, 0, shuffle=True)
    r0 = _loader(ds, 0, shuffle=True, rank=0, world_size=2)
    r1 = _loader(ds, 0, shuffle=True, rank=1, world_size=2)
    for epoch in (0, 1, 2):
        full = whole.batches(epoch)
        assert len(full) == 2 and len({i for b in full for i in b}) == 4       # one of five lines is dropped
        s0, s1 = r0.batches(epoch), r1.batches(epoch)
        assert len(s0) == len(s1) == len(r0) == 1
        assert not ({i for b in s0 for i in b} & {i for b in s1 for i in b})   # disjoint
        assert sorted(s0 + s1) == sorted(full)                                 # and together the epoch
    assert len({tuple(map(tuple, whole.batches(e))) for e in range(6)}) > 1    # the order depends on the epoch
    assert whole.batches(3) == _loader(ds, 2, shuffle=True).batches(3)         # and on nothing else
    # the shard a rank yields is the batch it was dealt
    r1.set_epoch(2)
    (got,) = list(r1)
    whole.set_epoch(2)
    both = list(whole)
    k = whole.batches(2).index(r1.batches(2)[0])
    torch.cuda.synchronize()
    for key in got:
        assert torch.equal(got[key], both[k][key]), key


def test_stereo_and_depth_keys(tree):
    from monodepth2_amd.datasets import KITTIDepthDataset
    ds = _dataset(tree, frame_ids=[0, "s"], cls=KITTIDepthDataset, load_depth=True)
    ld = _loader(ds, 2, with_depth=True)
    batches = list(ld)
    torch.cuda.synchronize()
    ld.close()
    for n, batch in enumerate(batches):
        assert batch["depth_gt"].shape == (2, 1, 375, 1242) and batch["depth_gt"].dtype == torch.float32
        for j, idx in enumerate(ld.batches(0)[n]):
            item = ds.parse(idx, epoch=0)
            sign = (-1 if item.side == "l" else 1) * (-1 if item.draw.do_flip else 1)
            assert float(batch["stereo_T"][j, 0, 3]) == pytest.approx(0.1 * sign)
            want = ds.get_depth(item.folder, item.frame_index, item.side, item.draw.do_flip)
            assert np.array_equal(batch["depth_gt"][j, 0].cpu().numpy(), want)
    with pytest.raises(ValueError, match="load_depth"):
        _loader(_dataset(tree), 0, with_depth=True)


def test_raw_depth_gt_from_the_velodyne_scans(tmp_path):
    """KITTIRAWDataset's depth_gt through the loader (what `--dataset kitti` validates
    on): per item kitti_utils.generate_depth_map at the calibrated size, PIL NEAREST to
    1242 x 375 (the identity for the 375 x 1242 rig, a resampling for the 370 x 1226 one),
    the item's flip.  Each batch mixes both rigs and both cameras."""
    from monodepth2_amd import kitti_utils as ku
    from monodepth2_amd.datasets import KITTIRAWDataset
    root = str(tmp_path)
    KT.write_tree(root)
    frames = KT.write_velodyne(root)
    lines = [KT.LINES[0], KT.LINES[3], KT.LINES[2], KT.LINES[1]]           # (rig 0 l, rig 1 r), (rig 0 r, rig 1 l)
    ds = KITTIRAWDataset(root, lines, H, W, FRAME_IDS, S, is_train=True, img_ext=".png", seed=5, load_depth=True)
    assert ds.load_depth
    flips = [ds.parse(i, epoch=0).draw.do_flip for i in range(4)]
    assert True in flips and False in flips, flips                       # both branches of the flip
    want = []
    for i in range(4):
        item = ds.parse(i, epoch=0)
        calib, scan = frames[[d for d, _ in KT.DRIVES].index(item.folder)]
        native = ku.generate_depth_map(calib, scan, ds.side_map[item.side])
        assert native.shape == KT.CALIBRATED[[d for d, _ in KT.DRIVES].index(item.folder)]
        assert np.count_nonzero(native) > 1000
        full = np.array(Image.fromarray(native).resize((1242, 375), Image.NEAREST))
        want.append(np.fliplr(full) if item.draw.do_flip else full)
    assert np.array_equal(want[0] if not flips[0] else np.fliplr(want[0]),
                          ku.generate_depth_map(*frames[0], 2))          # 375 x 1242: the map itself
    for threads in (0, 2):
        ld = _loader(ds, threads, with_depth=True)
        batches = list(ld)
        torch.cuda.synchronize()
        ld.close()
        assert len(batches) == 2
        for n, batch in enumerate(batches):
            got = batch["depth_gt"]
            assert got.shape == (2, 1, 375, 1242) and got.dtype == torch.float32 and got.is_cuda
            for j in range(2):
                assert np.array_equal(got[j, 0].cpu().numpy().view(np.uint32), want[2 * n + j].view(np.uint32)), (n, j)
    # one frame on its own is the batch's
    one = ds.get_depth(KT.DRIVES[1][0], 1, "r", flips[1])
    assert np.array_equal(one.cpu().numpy(), want[1])


def test_a_batch_larger_than_the_ring_was_sized_for(tmp_path):
    """The pinned ring is sized from the epoch's first batch; a later batch of much larger
    frames is staged in pageable memory and its slot grown: same bits as the oracle."""
    from monodepth2_amd.datasets import KITTIRAWDataset
    root = str(tmp_path)
    KT.write_tree(root)
    big = "2011_09_30/2011_09_30_drive_0003_sync"
    rng = np.random.default_rng(9)
    os.makedirs(os.path.join(root, big, "image_02/data"))
    for frame in range(3):
        Image.fromarray(KT.image(rng, 170, 330)).save(os.path.join(root, big, "image_02/data", "%010d.png" % frame))
    lines = KT.LINES[:2] + ["{} 1 l".format(big)] * 2 + KT.LINES[:2]
    ds = KITTIRAWDataset(root, lines, H, W, FRAME_IDS, S, is_train=True, img_ext=".png", seed=5)
    for threads in (0, 2):
        ld = _loader(ds, threads)
        batches = list(ld)
        torch.cuda.synchronize()
        ld.close()
        assert len(batches) == 3
        assert min(p.numel() for p in ld._pinned if p is not None) < 2 * 3 * 170 * 330 * 3   # the ring was too small
        for n, batch in enumerate(batches):
            for j in range(2):
                item = ds.parse(2 * n + j, epoch=0)
                d = item.draw
                jit = (d.order, d.brightness, d.contrast, d.saturation, d.hue) if d.do_color_aug else None
                for fid, path in zip(FRAME_IDS, item.paths):
                    color, caug = A.preprocess(np.asarray(Image.open(path).convert("RGB")), H, W, S, flip=d.do_flip,
                                               jitter=jit)
                    assert np.array_equal(batch[("color", fid, 0)][j].cpu().numpy(), color[0]), (n, j, fid)
                    assert np.array_equal(batch[("color_aug", fid, 0)][j].cpu().numpy(), caug[0]), (n, j, fid)


def test_a_failed_item_leaves_no_file_open(tree, monkeypatch):
    """If one item of a batch cannot be opened, the files already opened for the batch are
    closed before the error is raised."""
    from monodepth2_amd.datasets import KITTIRAWDataset
    opened = []
    real = Image.open

    def tracking(path, *a, **kw):
        im = real(path, *a, **kw)
        opened.append(im)
        return im

    monkeypatch.setattr(Image, "open", tracking)
    lines = [KT.LINES[0], "{} 2 l".format(KT.DRIVES[1][0])]                  # frame 3 does not exist
    ds = KITTIRAWDataset(tree, lines, H, W, FRAME_IDS, S, img_ext=".png")
    ld = _loader(ds, 0)
    with pytest.raises(FileNotFoundError, match="line 1"):
        list(ld)
    ld.close()
    assert len(opened) == 5 and all(im.fp is None for im in opened)       # 3 of item 0, 2 of item 1


def test_errors_reach_the_caller(tree, tmp_path):
    from monodepth2_amd.datasets import KITTIRAWDataset
    lines = KT.LINES[:2] + ["{} 2 l".format(KT.DRIVES[1][0]), KT.LINES[0]]     # frame 3 does not exist
    ds = KITTIRAWDataset(tree, lines, H, W, FRAME_IDS, S, img_ext=".png")
    for threads in (0, 2):
        ld = _loader(ds, threads)
        with pytest.raises(FileNotFoundError, match="line 2"):
            list(ld)
        ld.close()
