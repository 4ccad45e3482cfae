"""loader.BatchLoader(drop_last=False), the evaluation order: five lines of the tiny
KITTI-shaped tree (tests/kitti_tree.py) in batches of 2 give 2, 2, 1 items in list order,
each bit-equal to the PIL pipeline; the default loader is what it was."""
import numpy as np
import pytest
import torch
from PIL import Image

import kitti_tree as KT
from oracle import augment_oracle as A

pytestmark = pytest.mark.gpu

H, W = 64, 128


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_tail"))
    KT.write_tree(root)
    return root


def _dataset(root, frame_ids=(0,), num_scales=1):
    from monodepth2_amd.datasets import KITTIRAWDataset
    return KITTIRAWDataset(root, KT.LINES, H, W, list(frame_ids), num_scales, is_train=False, img_ext=".png")


def _pil(path, num_scales=1):
    """Pillow resize((W, H), LANCZOS) + to_tensor of the file, per scale."""
    color, _ = A.preprocess(np.asarray(Image.open(path).convert("RGB")), H, W, num_scales, flip=False, jitter=None)
    return color


@pytest.mark.parametrize("threads", [0, 2])
def test_the_tail_batch_is_produced_in_list_order(tree, threads):
    from monodepth2_amd.loader import BatchLoader
    ds = _dataset(tree)
    ld = BatchLoader(ds, 2, shuffle=False, drop_last=False, num_workers=threads)
    assert len(ld) == 3 and ld.batches(0) == [[0, 1], [2, 3], [4]]
    batches = list(ld)
    torch.cuda.synchronize()
    ld.close()
    assert [b[("color", 0, 0)].shape[0] for b in batches] == [2, 2, 1]
    assert ld.epoch == 1
    index = 0
    for batch in batches:
        color = batch[("color", 0, 0)]
        assert color.shape[1:] == (3, H, W) and color.dtype == torch.float32 and color.is_contiguous()
        assert batch[("K", 0)].shape == (color.shape[0], 4, 4)
        assert torch.equal(batch[("color_aug", 0, 0)], color)       # is_train False: no jitter, no flip
        for j in range(color.shape[0]):
            item = ds.parse(index)
            want = _pil(item.paths[0])[0]
            assert np.array_equal(color[j].cpu().numpy(), want), (index, item.line)
            # PIL directly, without the oracle's helper
            direct = np.asarray(Image.open(item.paths[0]).convert("RGB").resize((W, H), Image.LANCZOS))
            assert np.array_equal(color[j].cpu().numpy(), direct.transpose(2, 0, 1).astype(np.float32) / 255), index
            index += 1
    assert index == 5
    # a second epoch reuses both plans
    again = list(ld) if threads == 0 else None
    if again is not None:
        torch.cuda.synchronize()
        for x, y in zip(batches, again):
            assert torch.equal(x[("color", 0, 0)], y[("color", 0, 0)])


def test_two_frames_and_a_pyramid_in_the_tail(tree):
    """What evaluate_pose feeds ([0, 1]) and a four-scale pyramid: the tail's own plan has
    the loader's frames and scales."""
    from monodepth2_amd.loader import BatchLoader
    ds = _dataset(tree, frame_ids=(0, 1), num_scales=4)
    ld = BatchLoader(ds, 2, shuffle=False, drop_last=False, num_workers=0)
    batches = list(ld)
    torch.cuda.synchronize()
    ld.close()
    assert [b[("color", 1, 0)].shape[0] for b in batches] == [2, 2, 1]
    for n, batch in enumerate(batches):
        for j in range(batch[("color", 0, 0)].shape[0]):
            item = ds.parse(2 * n + j)
            for fid, path in zip((0, 1), item.paths):
                want = _pil(path, 4)
                for s in range(4):
                    assert np.array_equal(batch[("color", fid, s)][j].cpu().numpy(), want[s]), (n, j, fid, s)


def test_the_default_still_drops_the_partial_batch(tree):
    from monodepth2_amd.loader import BatchLoader
    ds = _dataset(tree)
    default = BatchLoader(ds, 2, shuffle=False, num_workers=0)
    explicit = BatchLoader(ds, 2, shuffle=False, num_workers=0, drop_last=True)
    whole = BatchLoader(ds, 2, shuffle=False, num_workers=0, drop_last=False)
    assert len(default) == len(explicit) == 2
    assert default.batches(0) == explicit.batches(0) == [[0, 1], [2, 3]] == whole.batches(0)[:2]
    a, b, c = list(default), list(explicit), list(whole)
    torch.cuda.synchronize()
    assert len(a) == len(b) == 2 and len(c) == 3
    for x, y, z in zip(a, b, c):
        assert x.keys() == y.keys() == z.keys()
        for k in x:
            assert torch.equal(x[k], y[k]) and torch.equal(x[k], z[k]), k
    assert default._tail_aug is None and whole._tail_aug is not None and whole._tail_aug.batch_size == 1
    # shuffled: the same permutation, the tail being what the default drops
    s_def = BatchLoader(ds, 2, shuffle=True, seed=5, num_workers=0)
    s_all = BatchLoader(ds, 2, shuffle=True, seed=5, num_workers=0, drop_last=False)
    for epoch in (0, 1):
        assert s_all.batches(epoch)[:2] == s_def.batches(epoch) and len(s_all.batches(epoch)[2]) == 1
    for ld in (default, explicit, whole, s_def, s_all):
        ld.close()


def test_more_than_one_rank_is_refused(tree):
    from monodepth2_amd.loader import BatchLoader
    with pytest.raises(ValueError, match="drop_last=False"):
        BatchLoader(_dataset(tree), 2, shuffle=False, drop_last=False, rank=1, world_size=2)
    BatchLoader(_dataset(tree), 2, shuffle=False, drop_last=True, rank=1, world_size=2).close()
