"""GPU tests of the pose-evaluation operator (csrc/traj.hip, pose_eval_ops.trajectory_ate)
and of evaluate_pose.predict_poses / evaluate.

Yardsticks: tests/pose_eval_case.py, the numpy fp64 restatement of md2_pose_ate in the
kernel's written order — compared bitwise, as uint64 views — and
tests/golden/pose_eval/pose_eval.npz, captured from the reference's own evaluate_pose.py,
within 8 x the floor measured when it was made (tests/test_pose_eval_abi.py states why 8).
Bitwise parity rests on the device's fp64 divide and sqrt being correctly rounded under
the default compiler flags and on nothing being contracted into an fma.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import pose_eval_case as pc
from monodepth2_amd.pose_eval_ops import trajectory_ate, workspace_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAR_FACTOR = 8


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def sequence(frames):
    """(pred (M-1,4,4) fp32, gt (M,3,4) fp64) of a synthetic drive of `frames` frames, the
    predictions through the CPU restatement of transformation_from_parameters."""
    from monodepth2_amd.layers import transformation_from_parameters
    gt = pc.parse_text(pc.drive_text(frames, seed=frames))
    aa, tr = pc.predictions(gt, seed=frames)
    pred = transformation_from_parameters(torch.from_numpy(aa), torch.from_numpy(tr)).numpy()
    assert pred.dtype == np.float32 and pred.shape == (frames - 1, 4, 4)
    return pred, gt


@functools.lru_cache(maxsize=None)
def expected(frames, track_length):
    """The restatement's (ates, stats) for `sequence(frames)`: computed once, shared."""
    pred, gt = sequence(frames)
    ates, stats = pc.trajectory_ate_np(pred, gt, track_length)
    ates.setflags(write=False), stats.setflags(write=False)
    return ates, stats


@functools.lru_cache(maxsize=None)
def golden():
    return pc.load_golden()


# M = 2: one snippet of two points; 5: every snippet truncated; 6: the first full snippet;
# 300: more than 256 snippets and no multiple of 256 (the strided part of the reduction)
SHAPES = [(2, 5), (5, 5), (6, 5), (300, 5), (6, 2), (6, 3), (300, 2), (300, 3)]


@pytest.mark.parametrize("frames,track_length", SHAPES)
def test_kernel_is_bit_equal_to_the_restatement(frames, track_length):
    pred, gt = sequence(frames)
    want_ates, want_stats = expected(frames, track_length)
    ates, stats = trajectory_ate(cuda(pred), cuda(gt), None, track_length)
    assert ates.shape == (frames - 1,) and stats.shape == (1, 2)
    assert ates.dtype == stats.dtype == torch.float64 and ates.is_cuda and stats.is_cuda
    got_a, got_s = ates.cpu().numpy(), stats.cpu().numpy()[0]
    with np.errstate(all="ignore"):
        print("frames", frames, "track", track_length, "max rel diff ates",
              np.max(np.abs(got_a - want_ates) / want_ates), "stats", got_s, want_stats)
    assert np.isfinite(want_ates).all() and want_ates.min() > 0
    assert np.array_equal(bits(got_a), bits(want_ates))
    assert np.array_equal(bits(got_s), bits(want_stats))


def test_batch_equals_single_sequences_and_list_form_equals_offsets_form():
    lengths = (2, 6, 300)
    preds, gts = zip(*(sequence(m) for m in lengths))
    singles = [trajectory_ate(cuda(p), cuda(g)) for p, g in zip(preds, gts)]
    pred_all = cuda(np.concatenate(preds))
    ates, stats = trajectory_ate(pred_all, [cuda(g) for g in gts])
    assert ates.shape == (sum(lengths) - 3,) and stats.shape == (3, 2)
    assert np.array_equal(bits(ates), bits(torch.cat([a for a, _ in singles])))
    assert np.array_equal(bits(stats), bits(torch.cat([s for _, s in singles])))
    for m, (_, s) in zip(lengths, singles):
        assert np.array_equal(bits(s[0]), bits(expected(m, 5)[1]))
    offsets = torch.tensor([0, 2, 8, 308], dtype=torch.int64)
    for off in (offsets, offsets.to(DEV)):          # validated on the host / the kernel's contract
        a2, s2 = trajectory_ate(pred_all, cuda(np.concatenate(gts)), off)
        assert np.array_equal(bits(a2), bits(ates)) and np.array_equal(bits(s2), bits(stats))
    with pytest.raises(ValueError, match="at least 2 frames"):
        trajectory_ate(pred_all, cuda(np.concatenate(gts)), torch.tensor([0, 1, 8, 308]))
    with pytest.raises(ValueError, match="float32"):
        trajectory_ate(pred_all.double(), cuda(np.concatenate(gts)), offsets)
    with pytest.raises(ValueError, match="float64"):
        trajectory_ate(pred_all, cuda(np.concatenate(gts)).float(), offsets)
    with pytest.raises(ValueError, match="predicted transforms"):
        trajectory_ate(pred_all[:-1], cuda(np.concatenate(gts)), offsets.to(DEV))


@pytest.mark.parametrize("s", range(len(pc.FRAMES)))
def test_kernel_reproduces_the_reference_golden(s):
    """The kernel on the golden's recorded pred_poses against the reference's ATEs, mean
    and std: within 8 x the measured floor (6.3e-12), the bar of the CPU restatement test."""
    g = golden()
    bar = BAR_FACTOR * float(g["floor"])
    ates, stats = trajectory_ate(cuda(g["pred_poses_%d" % s]), cuda(g["gt_%d" % s]))
    got = np.concatenate([ates.cpu().numpy(), stats.cpu().numpy()[0]])
    want = np.concatenate([g["ates_%d" % s], [g["mean_%d" % s], g["std_%d" % s]]])
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    print("sequence", s, "kernel vs golden", err, "bar", bar)
    assert err <= bar


@pytest.mark.parametrize("s", range(len(pc.FRAMES)))
def test_end_to_end_from_axisangle_and_translation(s):
    """Golden axisangle and translation through pose_ops.poses_to_transforms (csrc/pose.hip),
    then trajectory_ate, against the golden ATEs.  The transforms come from another
    implementation of transformation_from_parameters than the reference's, so the bar is the
    sensitivity of the ATEs, mean and std to one fp32 ulp in every element of pred_poses,
    measured on the CPU when the golden was made, times 4 (`ulp_bar` in the npz: 4.3e-5)."""
    from monodepth2_amd.pose_ops import poses_to_transforms
    g = golden()
    bar = float(g["ulp_bar"])
    aa, tr = cuda(g["axisangle_%d" % s]), cuda(g["translation_%d" % s])
    T = poses_to_transforms(aa[:, 0].unsqueeze(0), tr[:, 0].unsqueeze(0), [False])[0]
    assert T.shape == (pc.FRAMES[s] - 1, 4, 4) and T.dtype == torch.float32
    want_T = g["pred_poses_%d" % s]
    print("sequence", s, "max |T - reference T|", float(np.abs(T.cpu().numpy() - want_T).max()))
    ates, stats = trajectory_ate(T, cuda(g["gt_%d" % s]))
    got = np.concatenate([ates.cpu().numpy(), stats.cpu().numpy()[0]])
    want = np.concatenate([g["ates_%d" % s], [g["mean_%d" % s], g["std_%d" % s]]])
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    print("sequence", s, "end to end vs golden", err, "bar", bar)
    assert err <= bar


def test_identity_prediction_gives_nan_and_leaves_the_neighbour_alone():
    pred, gt = sequence(6)
    ident = pc.identity_poses(5)
    with np.errstate(all="ignore"):
        want_a, want_s = pc.trajectory_ate_np(ident, gt)
    assert np.isnan(want_a).all() and np.isnan(want_s).all()
    ates, stats = trajectory_ate(cuda(np.concatenate([ident, pred])), [cuda(gt), cuda(gt)])
    ates, stats = ates.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(ates[:5], want_a, equal_nan=True) and np.isnan(ates[:5]).all()
    assert np.array_equal(stats[0], want_s, equal_nan=True) and np.isnan(stats[0]).all()
    assert np.array_equal(bits(ates[5:]), bits(expected(6, 5)[0]))
    assert np.array_equal(bits(stats[1]), bits(expected(6, 5)[1]))


def test_bitwise_repeatable_and_capturable():
    lengths = (6, 300)
    preds, gts = zip(*(sequence(m) for m in lengths))
    pred, gt = cuda(np.concatenate(preds)), cuda(np.concatenate(gts))
    offsets = torch.tensor([0, 6, 306], dtype=torch.int64).to(DEV)
    a = trajectory_ate(pred, gt, offsets)
    b = trajectory_ate(pred, gt, offsets)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        trajectory_ate(pred, gt, offsets)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = trajectory_ate(pred, gt, offsets)
    replays = []
    for _ in range(2):
        out[0].fill_(-1.0), out[1].fill_(-1.0)
        graph.replay()
        replays.append((out[0].clone(), out[1].clone()))
    torch.cuda.synchronize()
    for r in replays:
        assert torch.equal(r[0].view(torch.int64), a[0].view(torch.int64))
        assert torch.equal(r[1].view(torch.int64), a[1].view(torch.int64))


def test_caller_workspace_with_garbage():
    pred, gt = sequence(300)
    need = workspace_bytes(1, 300)
    assert need >= 96 * 299 and need % 256 == 0
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    ates, stats = trajectory_ate(cuda(pred), cuda(gt), workspace=ws)
    assert np.array_equal(bits(ates), bits(expected(300, 5)[0]))
    assert np.array_equal(bits(stats[0]), bits(expected(300, 5)[1]))
    with pytest.raises(ValueError, match="workspace"):
        trajectory_ate(cuda(pred), cuda(gt), workspace=ws[:need - 256])


def test_predict_poses_no_worse_than_stock_modules(monkeypatch):
    from monodepth2_amd import bn_ops, conv_ops, networks, stem_ops
    from monodepth2_amd.evaluate_pose import predict_poses
    from monodepth2_amd.layers import transformation_from_parameters
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False, 2)
    dec = networks.PoseDecoder(enc.num_ch_enc, 1, 2)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(5, 3, 64, 128, generator=g)

    def pairs(x):
        return torch.cat([x[:-1], x[1:]], 1)

    with torch.no_grad():
        e64, d64 = copy.deepcopy(enc).double().eval(), copy.deepcopy(dec).double().eval()
        aa, tr = d64([e64(pairs(images.double()))])
        exact = transformation_from_parameters(aa[:, 0], tr[:, 0])
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV).to(memory_format=torch.channels_last)
    enc.train()
    dec.eval()
    ours = predict_poses(enc, dec, images.to(DEV))
    assert enc.training and not dec.training               # flags restored
    assert ours.shape == (4, 4, 4) and ours.dtype == torch.float32 and ours.is_cuda
    two = predict_poses(enc, dec, images.to(DEV), batch_size=3)   # batches of 3 + 1 pairs
    # the same pairs in other batches: eval-mode BatchNorm, so only the convolutions' choice of
    # kernel per batch size can differ, by fp32 rounding of values of at most 1
    assert torch.allclose(two, ours, atol=1e-5)
    for mod in (bn_ops, conv_ops, stem_ops):               # stock: every fused path off
        monkeypatch.setattr(mod, "ENABLED", False)
    monkeypatch.setattr(stem_ops, "FWD_ENABLED", False)
    enc.eval()
    with torch.no_grad():
        aa, tr = dec([enc(pairs(images.to(DEV)))])
        ref = transformation_from_parameters(aa[:, 0], tr[:, 0])
    e_ours = (ours.cpu().double() - exact).abs().max().item()
    e_ref = (ref.cpu().double() - exact).abs().max().item()
    print("predict_poses: e_ours", e_ours, "e_ref (stock fp32 modules)", e_ref)
    assert e_ours <= 3 * e_ref


@pytest.mark.parametrize("s", range(len(pc.FRAMES)))
def test_evaluate_from_files(s, tmp_path, capsys):
    """evaluate(opt) as `python -m monodepth2_amd.evaluate_pose` runs it: the golden's pose
    text as --gt_poses, its pred_poses as --ext_poses_to_eval; the reference's line on
    stdout, nothing written."""
    from monodepth2_amd.evaluate_pose import evaluate
    from monodepth2_amd.options import MonodepthOptions
    g = golden()
    (tmp_path / "09.txt").write_text(str(g["pose_text_%d" % s]))
    np.save(tmp_path / "poses.npy", g["pred_poses_%d" % s])
    before = sorted(p.name for p in tmp_path.iterdir())
    res = evaluate(MonodepthOptions().parse(["--eval_split", "odom_9", "--ext_poses_to_eval", str(tmp_path / "poses.npy"),
                                             "--gt_poses", str(tmp_path / "09.txt"),
                                             "--load_weights_folder", str(tmp_path)]))
    text = capsys.readouterr().out
    assert str(g["line_%d" % s]) in text
    assert res["ates"].shape == (pc.FRAMES[s] - 1,) and res["ates"].dtype == np.float64
    assert abs(res["mean"] - float(g["mean_%d" % s])) <= BAR_FACTOR * float(g["floor"]) * res["mean"]
    assert sorted(p.name for p in tmp_path.iterdir()) == before


def test_evaluate_from_images_saves_poses(tmp_path, capsys):
    """evaluate(opt, images): checkpoint from --load_weights_folder, predictions saved there
    as poses.npy (evaluate_pose.py:127-128), and that file evaluates to the same line."""
    from monodepth2_amd import networks
    from monodepth2_amd.evaluate_pose import evaluate
    from monodepth2_amd.options import MonodepthOptions
    torch.manual_seed(0)
    enc = networks.ResnetEncoder(18, False, 2)
    dec = networks.PoseDecoder(enc.num_ch_enc, 1, 2)
    torch.save(enc.state_dict(), tmp_path / "pose_encoder.pth")
    torch.save(dec.state_dict(), tmp_path / "pose.pth")
    (tmp_path / "10.txt").write_text(pc.drive_text(5, seed=5))
    images = torch.rand(5, 3, 64, 128, generator=torch.Generator().manual_seed(2))
    args = ["--eval_split", "odom_10", "--gt_poses", str(tmp_path / "10.txt"), "--load_weights_folder", str(tmp_path)]
    res = evaluate(MonodepthOptions().parse(args), images)
    first = capsys.readouterr().out
    saved = np.load(tmp_path / "poses.npy")
    assert saved.shape == (4, 4, 4) and saved.dtype == np.float32
    assert "Trajectory error: {:0.3f}, std: {:0.3f}".format(res["mean"], res["std"]) in first
    assert "-> Predictions saved to" in first
    again = evaluate(MonodepthOptions().parse(args + ["--ext_poses_to_eval", str(tmp_path / "poses.npy")]))
    assert np.array_equal(bits(again["ates"]), bits(res["ates"]))
