"""CPU-side checks of the 16-bit depth export (md2_depth_export16, csrc/eval.hip) and of the
evaluators' routes from --data_path: struct layout, every refusal and its message (no
kernel is launched), the data fixtures under tests/golden/splits/, the numpy restatement
of the export (tests/export16_case.py) in fp32 against fp64, and the evaluators' new
refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib
from monodepth2_amd.build import build
from monodepth2_amd.eval_ops import benchmark_depth_maps, check_depth16, depth16_desc, write_benchmark_pngs

import export16_case as xc

HERE = os.path.dirname(os.path.abspath(__file__))
SPLITS = os.path.join(HERE, "golden", "splits")


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def test_struct_layout_and_abi(L):
    D = _lib.Depth16Desc
    assert ctypes.sizeof(D) == 72
    assert (D.batch.offset, D.in_height.offset, D.in_width.offset, D.out_height.offset) == (0, 4, 8, 12)
    assert (D.out_width.offset, D.flags.offset, D.min_depth.offset, D.max_depth.offset) == (16, 20, 24, 32)
    assert (D.scale_factor.offset, D.clip_max.offset, D.quant.offset, D.reserved.offset) == (40, 48, 56, 64)
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert {"md2_depth_export16", "md2_depth_export16_check"} <= set(_lib.EXPORTS)
    assert hasattr(L, "md2_depth_export16") and hasattr(L, "md2_depth_export16_check")
    assert _lib.DEPTH16_POST_PROCESS == 1


def desc(**kw):
    args = dict(batch=2, in_hw=(24, 80), out_hw=(352, 1216))
    args.update(kw)
    return depth16_desc(**args)


INF, NAN = float("inf"), float("nan")
BAD = [
    (dict(batch=0), "must be positive"),
    (dict(batch=-1), "must be positive"),
    (dict(in_hw=(0, 80)), "must be positive"),
    (dict(in_hw=(24, -5)), "must be positive"),
    (dict(out_hw=(0, 1216)), "must be positive"),
    (dict(out_hw=(352, 0)), "must be positive"),
    (dict(batch=65536), "65535"),                       # images are grid.y
    (dict(out_hw=(2 ** 16, 2 ** 15)), "2^31"),
    (dict(in_hw=(2 ** 16, 2 ** 15)), "2^31"),
    (dict(batch=2, out_hw=(2 ** 15, 2 ** 15)), "2^31"),
    (dict(batch=4, in_hw=(2 ** 15, 2 ** 14)), "2^31"),
    (dict(batch=1, out_hw=(2 ** 31 - 1, 2 ** 31 - 1)), "2^31"),   # the products are formed in 64 bits
    (dict(scale_factor=0.0), "positive and finite"),
    (dict(scale_factor=-5.4), "positive and finite"),
    (dict(scale_factor=INF), "positive and finite"),
    (dict(scale_factor=NAN), "positive and finite"),
    (dict(clip_max=0.0), "positive and finite"),
    (dict(clip_max=INF), "positive and finite"),
    (dict(clip_max=NAN), "positive and finite"),
    (dict(quant=0.0), "positive and finite"),
    (dict(quant=-256.0), "positive and finite"),
    (dict(quant=INF), "positive and finite"),
    (dict(quant=NAN), "positive and finite"),
    (dict(clip_max=80.0, quant=1024.0), "65535"),       # 81920 does not fit 16 bits
    (dict(clip_max=256.0, quant=256.0), "65535"),       # 65536: one past
    (dict(min_depth=0.0), "min_depth"),
    (dict(min_depth=100.0, max_depth=100.0), "min_depth"),
    (dict(max_depth=NAN), "min_depth"),
]


def call(L, d, ptrs):
    return L.md2_depth_export16(ctypes.byref(d) if d is not None else None, *ptrs, None)


@pytest.mark.parametrize("kw,msg", BAD)
def test_invalid_desc_is_refused_with_a_message(L, kw, msg):
    d = desc(**kw)
    dummy = ctypes.c_void_p(256)   # non-NULL, never dereferenced: the desc is refused first
    assert L.md2_depth_export16_check(ctypes.byref(d)) == -1
    assert msg in L.md2_last_error().decode()
    assert call(L, d, [dummy] * 3) == -1
    assert msg in L.md2_last_error().decode() and "depth_export16" in L.md2_last_error().decode()
    with pytest.raises(RuntimeError, match="md2_depth_export16_check"):
        check_depth16(d)


def test_the_largest_legal_values_are_accepted(L):
    for kw in (dict(batch=65535, in_hw=(1, 1), out_hw=(1, 1)), dict(batch=1, out_hw=(2 ** 15, 2 ** 16 - 1)),
               dict(clip_max=255.99609375, quant=256.0),   # 65535 exactly
               dict(clip_max=65535.0, quant=1.0), dict(min_depth=1.0, max_depth=INF), dict(post_process=True)):
        assert L.md2_depth_export16_check(ctypes.byref(desc(**kw))) == 0, kw
        check_depth16(desc(**kw))


def test_null_desc_operands_flags_and_alignment(L):
    x = ctypes.c_void_p(256)
    assert L.md2_depth_export16_check(None) == -1
    assert "NULL desc" in L.md2_last_error().decode()
    assert call(L, None, [x] * 3) == -1
    assert "NULL desc" in L.md2_last_error().decode()
    d = desc()
    for hole in (0, 2):             # disp, out; disp_flipped (1) is optional without the flag
        args = [x] * 3
        args[hole] = None
        assert call(L, d, args) == -1
        assert "NULL operand" in L.md2_last_error().decode()
    assert call(L, desc(post_process=True), [x, None, x]) == -1
    assert "needs disp_flipped" in L.md2_last_error().decode()
    assert call(L, d, [x, x, ctypes.c_void_p(257)]) == -1
    assert "2-byte aligned" in L.md2_last_error().decode()
    for flags in (2, 4, 1 << 31, 3):
        d = desc()
        d.flags = flags
        assert L.md2_depth_export16_check(ctypes.byref(d)) == -1
        assert "unknown flags" in L.md2_last_error().decode()
        assert call(L, d, [x] * 3) == -1
        assert "unknown flags" in L.md2_last_error().decode()
    d = desc()
    d.reserved = 1
    assert call(L, d, [x] * 3) == -1
    assert "reserved" in L.md2_last_error().decode()


def test_the_python_operators_have_no_cpu_fallback_and_check_their_input(tmp_path):
    with pytest.raises(RuntimeError, match="GPU only"):
        benchmark_depth_maps(torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        benchmark_depth_maps(np.zeros((1, 1, 4, 4), np.float32))
    with pytest.raises(ValueError, match="int16 or uint16"):
        write_benchmark_pngs(np.zeros((1, 4, 4), np.float32), str(tmp_path))
    with pytest.raises(ValueError, match="int16 or uint16"):
        write_benchmark_pngs(np.zeros((4, 4), np.uint16), str(tmp_path))


def test_write_benchmark_pngs_round_trips_on_the_host(tmp_path):
    """The int16 storage holds uint16 bit patterns: values above 32767 come back as written."""
    from PIL import Image
    maps = np.array([[[0, 1, 20480], [32767, 32768, 65535]], [[7, 8, 9], [10, 11, 12]]], np.uint16)
    paths = write_benchmark_pngs(torch.from_numpy(maps.view(np.int16)), str(tmp_path / "out"), start=3)
    assert [os.path.basename(p) for p in paths] == ["0000000003.png", "0000000004.png"]
    for p, m in zip(paths, maps):
        with Image.open(p) as im:
            assert im.mode == "I;16" and im.size == (3, 2)
            assert np.array_equal(np.asarray(im), m)


def test_the_id_table_fixture():
    ids = np.load(os.path.join(SPLITS, "benchmark", "eigen_to_benchmark_ids.npy"))
    assert ids.shape == (652,) and ids.dtype == np.int64
    assert (np.diff(ids) > 0).all() and ids[0] >= 0 and ids[-1] < 697


@pytest.mark.parametrize("seq,count", [(9, 1590), (10, 1200)])
def test_the_odometry_lists_parse(seq, count):
    from monodepth2_amd.datasets import KITTIOdomDataset, readlines
    lines = readlines(os.path.join(SPLITS, "odom", "test_files_{:02d}.txt".format(seq)))
    assert len(lines) == count
    ds = KITTIOdomDataset("/data", lines, 192, 640, [0, 1], 1, is_train=False)
    for k in range(len(lines)):
        item = ds.parse(k)
        assert item.paths == ["/data/sequences/{:02d}/image_2/{:06d}.jpg".format(seq, k + d) for d in (0, 1)], lines[k]
        assert not item.draw.do_flip and not item.draw.do_color_aug


@pytest.fixture(scope="module")
def straddle():
    return xc.straddling_inputs()


@pytest.mark.parametrize("pp", [True, False])
def test_the_fp32_formulation_stays_within_one_count_of_fp64(straddle, pp):
    sig, sigf = straddle
    flipped = sigf if pp else None
    x64, depth = xc.export16_values(sig, flipped, (352, 1216), np.float64)
    x32, _ = xc.export16_values(sig, flipped, (352, 1216), np.float32)
    a, b = x64.astype(np.uint16), x32.astype(np.uint16)
    near = np.abs(x64 - np.rint(x64)) <= xc.DELTA
    unclipped = depth < 80.0
    print("pp" if pp else "plain", "near", int((near & unclipped).sum()), "of", x64.size,
          "image 1 clipped", float((depth[1] >= 80.0).mean()),
          "max |fp32 - fp64| counts", float(np.abs(x32.astype(np.float64) - x64).max()),
          "pixels that disagree", float((a != b).mean()))
    assert x64.size == 1284096
    assert 0.3 < (depth[1] >= 80.0).mean() < 0.6 and (depth[0] < 80.0).all() and (depth[2] < 80.0).all()
    assert np.abs(a.astype(np.int64) - b.astype(np.int64)).max() <= 1
    assert np.abs(x32.astype(np.float64) - x64).max() < 0.1
    assert (near & unclipped).sum() <= xc.MAX_EXCLUDED * unclipped.sum()
    assert (a[depth >= 80.0 * (1 + xc.CLIP_MARGIN)] == 20480).all()
    assert np.array_equal(xc.export16_np(sig, flipped, (352, 1216), np.float64), a)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_the_three_edge_values_in_the_restatement(dt):
    """Already-scaled input (min_depth 1, max_depth inf): constant images of 0, a negative
    value, NaN and 0.5 resize to themselves."""
    sig = np.empty((4, 1, 3, 5), np.float32)
    for b, v in enumerate((0.0, -0.25, np.nan, 0.5)):
        sig[b] = v
    got = xc.export16_np(sig, None, (4, 7), dt, min_depth=1.0, max_depth=float("inf"))
    assert (got[0] == 20480).all() and (got[1] == 0).all() and (got[2] == 0).all()
    assert (got[3] == int(5.4 / 0.5 * 256)).all()


def parse(argv):
    from monodepth2_amd.options import MonodepthOptions
    return MonodepthOptions().parse(argv)


@pytest.fixture
def no_gpu(monkeypatch):
    """The refusals below come before the device is asked for; if one did not, this makes
    the test fail with its own message instead of a HIP initialisation error."""
    def refuse():
        raise AssertionError("the refusal must come before the device is used")
    monkeypatch.setattr(torch.cuda, "current_device", refuse)


def test_depth_from_data_path_names_split_dir_when_the_list_is_missing(tmp_path, no_gpu):
    from monodepth2_amd.evaluate_depth import evaluate
    with pytest.raises(FileNotFoundError, match="--split_dir") as e:
        evaluate(parse(["--eval_mono", "--data_path", str(tmp_path), "--split_dir", str(tmp_path / "nowhere"),
                        "--load_weights_folder", str(tmp_path)]))
    assert "nowhere" in str(e.value) and "test_files.txt" in str(e.value)
    with pytest.raises(FileNotFoundError, match="--split_dir"):      # the default location ships no list
        evaluate(parse(["--eval_mono", "--data_path", str(tmp_path), "--load_weights_folder", str(tmp_path)]))


def test_benchmark_split_refusals(tmp_path, no_gpu):
    from monodepth2_amd.evaluate_depth import evaluate
    with pytest.raises(SystemExit, match="cannot be read from --data_path"):
        evaluate(parse(["--eval_mono", "--eval_split", "benchmark", "--data_path", str(tmp_path),
                        "--load_weights_folder", str(tmp_path)]))
    with pytest.raises(SystemExit, match="--eval_out_dir or --load_weights_folder"):
        evaluate(parse(["--eval_mono", "--eval_split", "benchmark", "--ext_disp_to_eval", str(tmp_path / "d.npy")]))


def test_a_missing_id_table_names_its_flag(tmp_path, no_gpu):
    from monodepth2_amd.evaluate_depth import evaluate
    np.save(tmp_path / "d.npy", np.zeros((697, 4, 8), np.float32))
    with pytest.raises(SystemExit, match="--eigen_to_benchmark_ids") as e:
        evaluate(parse(["--eval_mono", "--eval_eigen_to_benchmark", "--ext_disp_to_eval", str(tmp_path / "d.npy"),
                        "--eigen_to_benchmark_ids", str(tmp_path / "nowhere.npy")]))
    assert "nowhere.npy" in str(e.value)
    with pytest.raises(SystemExit, match="--eigen_to_benchmark_ids"):   # the default location ships no table
        evaluate(parse(["--eval_mono", "--eval_eigen_to_benchmark", "--ext_disp_to_eval", str(tmp_path / "d.npy")]))


def test_a_checkpoint_without_its_feed_size_is_refused(tmp_path):
    from monodepth2_amd import networks
    from monodepth2_amd.evaluate_depth import load_networks
    enc = networks.ResnetEncoder(18, False)
    dec = networks.DepthDecoder(enc.num_ch_enc)
    torch.save(enc.state_dict(), tmp_path / "encoder.pth")
    torch.save(dec.state_dict(), tmp_path / "depth.pth")
    assert load_networks(str(tmp_path), 18, "cpu")[2] is None
    torch.save(dict(enc.state_dict(), height=64, width=128), tmp_path / "encoder.pth")
    assert load_networks(str(tmp_path), 18, "cpu")[2] == (64, 128)


def test_pose_from_data_path_names_split_dir_when_the_list_is_missing(tmp_path, no_gpu):
    from monodepth2_amd.evaluate_pose import evaluate
    (tmp_path / "09.txt").write_text("1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 1\n")
    with pytest.raises(FileNotFoundError, match="--split_dir") as e:
        evaluate(parse(["--eval_split", "odom_9", "--gt_poses", str(tmp_path / "09.txt"),
                        "--split_dir", str(tmp_path / "nowhere")]))
    assert "test_files_09.txt" in str(e.value)


def test_the_new_refusals_are_still_not_implemented_errors():
    """The command lines the evaluators refused with NotImplementedError before these routes
    existed still raise one (a caller that caught it keeps working), now with the type that
    says what to do: a file to provide, or a usage error that exits."""
    from monodepth2_amd.options import EvalRefused, SplitListMissing
    assert issubclass(SplitListMissing, FileNotFoundError) and issubclass(SplitListMissing, NotImplementedError)
    assert issubclass(EvalRefused, SystemExit) and issubclass(EvalRefused, NotImplementedError)
    assert str(SplitListMissing("a b")) == "a b" and EvalRefused("usage").code == "usage"


def test_the_loader_refuses_the_tail_on_more_than_one_rank():
    """drop_last=False is the evaluation order: refused for world_size > 1 before anything
    touches the device."""
    from monodepth2_amd.loader import BatchLoader
    with pytest.raises(ValueError, match="drop_last=False"):
        BatchLoader(None, 2, shuffle=False, drop_last=False, rank=0, world_size=2)
