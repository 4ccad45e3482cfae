"""`python -m monodepth2_amd.train --log_images` end to end on the tiny KITTI-shaped tree:
contact sheets for train and val at the log steps, equal to the panel rebuilt from the same
step's tensors (tests/logpanel_case.py), also from a replayed hipGraph's static tensors; no
pictures without the flag or on another rank."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import kitti_tree as KT
import logpanel_case as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti"))
    KT.write_tree(root)
    KT.write_velodyne(root)
    KT.write_splits(os.path.join(root, "splits"))
    return root


def _argv(tree, log_dir, name, *extra):
    return ["--data_path", tree, "--split_dir", os.path.join(tree, "splits"), "--log_dir", str(log_dir),
            "--model_name", name, "--height", "64", "--width", "128", "--batch_size", "2", "--num_epochs", "1",
            "--log_frequency", "1", "--png", "--weights_init", "scratch", "--num_workers", "2", *extra]


FILES = sorted(["layout.json"] + ["step_{:07d}_{}.png".format(s, j) for s in (0, 1) for j in (0, 1)])


@pytest.fixture
def spy(monkeypatch):
    """Records, per log_images call, the sheet the numpy restatement builds from the tensors
    the call was given (the warps from md2_generate_images)."""
    from monodepth2_amd.hotpath import HotPathConfig, generate_images
    from monodepth2_amd.trainer import Trainer
    seen = {}
    real = Trainer.log_images

    def log_images(self, mode, inputs, outputs, step=None):
        panel = real(self, mode, inputs, outputs, step)
        if panel is None:
            return None
        if self.use_graph and mode == "train":
            inputs = self.static_inputs
        with torch.no_grad():
            K, inv_K = self._intrinsics(inputs)
            T = self._stacked_T(inputs, outputs)
            cfg = self.hot
            if cfg.t_per_scale:
                T, cfg = T[0], HotPathConfig(**{**cfg.__dict__, "t_per_scale": False})
            gen = generate_images(cfg, [outputs[("disp", s)] for s in range(4)], self._colors(inputs), K, inv_K,
                                  T, want_depth=False, want_sample=False)["color"]
        seen[(mode, step)] = (lc.expected_sheet(panel.layout, self.opt.frame_ids, inputs, outputs, gen, 2),
                              panel.layout, panel.stats.cpu().numpy())
        return panel

    monkeypatch.setattr(Trainer, "log_images", log_images)
    return seen


def _check_run(root, seen):
    for mode in ("train", "val"):
        folder = root / mode / "images"
        assert sorted(os.listdir(folder)) == FILES, mode
        with open(folder / "layout.json") as f:
            layout = {k: tuple(v) for k, v in json.load(f).items()}
        for step in (0, 1):
            want, (SH, SW, tags), stats = seen[(mode, step)]
            assert layout == tags
            assert list(tags) == lc.reference_tags([0, -1, 1], range(4), 2, False, False)
            for j in (0, 1):
                with Image.open(folder / "step_{:07d}_{}.png".format(step, j)) as im:
                    assert im.mode == "RGB" and im.size == (SW, SH)
                    got = np.asarray(im)
                assert np.array_equal(got, want[j]), (mode, step, j)
                for s in range(4):
                    y, x, h, w = tags["disp_{}/{}".format(s, j)]
                    tile = got[y:y + h, x:x + w]
                    assert np.isfinite(stats[j, s]).all() and stats[j, s, 1] > stats[j, s, 0]
                    assert tile.min() == 0 and tile.max() == 255      # finite and not constant: the full range
                y, x, h, w = tags["color_pred_-1_0/{}".format(j)]
                assert len(np.unique(got[y:y + h, x:x + w])) > 8


def test_log_images_writes_the_panels_of_the_log_steps(tree, tmp_path, spy):
    from monodepth2_amd import train
    tr = train.main(_argv(tree, tmp_path, "run", "--log_images"))
    assert tr.step == 2 and not tr.opt.materialize_images
    assert sorted(spy) == [("train", 0), ("train", 1), ("val", 0), ("val", 1)]
    _check_run(tmp_path / "run", spy)
    # a rank other than 0 runs the same steps and writes nothing
    loaders = train.build_loaders(tr.opt, tr)
    tr.rank, tr.opt.num_epochs = 1, 2
    tr.log_path = str(tmp_path / "rank1")
    tr.train(loaders[0], loaders[1])
    for ld in loaders:
        ld.close()
    assert tr.step == 4 and not os.path.exists(tr.log_path)
    assert tr.log_images("train", {}, {}) is None


def test_log_images_reads_a_replayed_graphs_static_outputs(tree, tmp_path, spy):
    from monodepth2_amd import train
    tr = train.main(_argv(tree, tmp_path, "graph", "--log_images", "--hip_graph"))
    assert tr.step == 2 and tr.graph is not None
    _check_run(tmp_path / "graph", spy)
    assert not np.array_equal(spy[("train", 0)][0], spy[("train", 1)][0])


def test_without_the_flag_nothing_is_written(tree, tmp_path, spy):
    from monodepth2_amd import train
    tr = train.main(_argv(tree, tmp_path, "plain"))
    assert tr.step == 2 and not spy
    for mode in ("train", "val"):
        assert os.listdir(tmp_path / "plain" / mode) == ["scalars.jsonl"]
