"""`python -m monodepth2_amd.train` end to end on a tiny KITTI-shaped tree: the loader,
the mixed-size GPU input pipeline, Trainer.train's logging rule, scalars and checkpoints."""
import json
import math
import os

import pytest
import torch

import kitti_tree as KT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti"))
    KT.write_tree(root)
    KT.write_velodyne(root)   # scans and calibration: the validation batches carry depth_gt
    KT.write_splits(os.path.join(root, "splits"))
    return root


def _argv(tree, log_dir, name, *extra):
    return ["--data_path", tree, "--split_dir", os.path.join(tree, "splits"), "--log_dir", str(log_dir),
            "--model_name", name, "--height", "64", "--width", "128", "--batch_size", "2", "--num_epochs", "1",
            "--log_frequency", "1", "--png", "--weights_init", "scratch", "--num_workers", "2", *extra]


def _scalars(path):
    with open(path) as f:
        return [json.loads(line) for line in f]


def test_train_run_logs_saves_and_resumes(tree, tmp_path, capsys):
    from monodepth2_amd import train
    tr = train.main(_argv(tree, tmp_path, "run"))
    assert tr.step == 2 and tr.epoch == 1             # five lines, batch 2: two steps
    models = tmp_path / "run" / "models"
    for f in ("weights_0/encoder.pth", "weights_0/depth.pth", "weights_0/pose.pth", "weights_0/adam.pth", "opt.json"):
        assert (models / f).is_file(), f
    for mode in ("train", "val"):
        rows = _scalars(tmp_path / "run" / mode / "scalars.jsonl")
        assert [r["step"] for r in rows] == [0, 1] and all(r["epoch"] == 0 for r in rows)   # one line per log step
        for r in rows:
            assert math.isfinite(r["loss"]) and all(math.isfinite(r["loss/{}".format(s)]) for s in range(4))
            # the validation monitor ran on ground truth projected from the scans
            assert ("de/abs_rel" in r) == (mode == "val") and (mode == "train" or math.isfinite(r["da/a1"]))
    saved = {n: {k: v.clone() for k, v in m.state_dict().items()} for n, m in tr.models.items()}
    # a second run starts from the saved parameters
    again = train.main(_argv(tree, tmp_path, "resume", "--load_weights_folder", str(models / "weights_0"),
                             "--num_epochs", "0"))
    assert again.step == 0
    for n, m in again.models.items():
        for k, v in m.state_dict().items():
            assert torch.equal(v, saved[n][k]), (n, k)
    on_disk = torch.load(models / "weights_0" / "encoder.pth", map_location="cpu", weights_only=True)
    assert on_disk["height"] == 64 and on_disk["width"] == 128
    # and trains on from them
    again.opt.num_epochs = 1
    loaders = train.build_loaders(again.opt, again)
    again.train(loaders[0], None)
    assert again.step == 2 and math.isfinite(_scalars(tmp_path / "resume" / "train" / "scalars.jsonl")[-1]["loss"])
    assert "examples/s" in capsys.readouterr().out
    # a rank other than 0 runs the same steps, prints nothing and writes nothing: with one
    # process per GPU every rank would otherwise open the same opt.json, scalars and
    # checkpoint files at once
    again.rank, again.opt.num_epochs, again.opt.save_frequency = 1, 2, 1
    again.log_path = str(tmp_path / "rank1")
    again.train(loaders[0], loaders[1])
    assert again.step == 4 and again.epoch == 2
    assert not os.path.exists(again.log_path)
    assert "examples/s" not in capsys.readouterr().out
    for ld in loaders:
        ld.close()


def test_train_run_with_hip_graph(tree, tmp_path):
    from monodepth2_amd import train
    tr = train.main(_argv(tree, tmp_path, "graph", "--hip_graph"))
    assert tr.step == 2 and tr.graph is not None
    rows = _scalars(tmp_path / "graph" / "train" / "scalars.jsonl")
    assert len(rows) == 2 and all(math.isfinite(r["loss"]) for r in rows)
    for p in tr.parameters_to_train:
        assert bool(torch.isfinite(p).all())


def test_missing_split_dir_says_what_to_pass(tree, tmp_path):
    from monodepth2_amd import train
    with pytest.raises(FileNotFoundError, match="--split_dir"):
        train.main(["--data_path", tree, "--split_dir", str(tmp_path / "nowhere"), "--log_dir", str(tmp_path),
                    "--height", "64", "--width", "128", "--batch_size", "2", "--weights_init", "scratch"])
