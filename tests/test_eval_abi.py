"""CPU-side checks of the depth-evaluation ABI (md2_depth_eval, ABI 24): struct size,
argument validation and its messages, workspace sizes — no kernel is launched — and the
pin of the tests' numpy restatement (tests/eval_case.py) to the golden captured from the
reference's own Trainer.compute_depth_losses."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib
from monodepth2_amd.build import build
from monodepth2_amd.eval_ops import eigen_crop, eval_desc

import eval_case


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def test_struct_size_and_abi(L):
    assert ctypes.sizeof(_lib.EvalDesc) == 72
    assert _lib.EvalDesc.flags.offset == 36 and _lib.EvalDesc.min_depth.offset == 40
    assert _lib.EvalDesc.eval_min.offset == 56 and _lib.EvalDesc.scale_factor.offset == 64
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION


def test_eigen_crop_matches_the_trainers_constants():
    assert eigen_crop(375, 1242) == (153, 371, 44, 1197)   # trainer.py:514
    assert eigen_crop(37, 124) == eval_case.eigen_crop(37, 124)


BAD = [
    (dict(batch=0), "positive"),
    (dict(height=0), "positive"),
    (dict(width=-3), "positive"),
    (dict(gt_height=0), "positive"),
    (dict(gt_width=0), "positive"),
    (dict(batch=4611, gt_height=375, gt_width=1242), "too large"),                 # > 2^31 gt pixels
    (dict(batch=1, gt_height=1, gt_width=2 ** 31 - 10000, crop=None), "too large"),   # within a grid stride of 2^31
    (dict(batch=60000, height=1000, width=1000, gt_height=2, gt_width=2, crop=None), "too large"),
    (dict(batch=65536, gt_height=2, gt_width=2, crop=None), "65535"),   # images are grid.y
    (dict(crop=(0, 38, 0, 124)), "crop"),
    (dict(crop=(0, 37, -1, 124)), "crop"),
    (dict(crop=(0, 37, 0, 125)), "crop"),
    (dict(crop=(20, 20, 0, 124)), "crop"),
    (dict(crop=(0, 37, 60, 50)), "crop"),
    (dict(min_depth=0.0), "min_depth"),
    (dict(min_depth=100.0, max_depth=0.1), "min_depth"),
    (dict(eval_min=0.0), "eval_min"),
    (dict(eval_min=80.0, eval_max=1e-3), "eval_min"),
    (dict(scale_factor=0.0), "scale_factor"),
    (dict(scale_factor=float("inf")), "scale_factor"),
    (dict(scale_factor=float("nan")), "scale_factor"),
]


def desc(**kw):
    args = dict(batch=3, height=24, width=80, gt_height=37, gt_width=124)
    args.update(kw)
    return eval_desc(**args)


@pytest.mark.parametrize("kw,msg", BAD)
def test_invalid_desc_is_refused_with_a_message(L, kw, msg):
    d = desc(**kw)
    dummy = ctypes.c_void_p(256)   # non-NULL, never dereferenced: the desc is refused first
    assert L.md2_depth_eval_workspace_bytes(ctypes.byref(d)) == 0
    assert msg in L.md2_last_error().decode()
    assert L.md2_depth_eval(ctypes.byref(d), dummy, dummy, dummy, dummy, dummy, None) == -1
    assert msg in L.md2_last_error().decode()


def test_null_desc_and_operands(L):
    assert L.md2_depth_eval_workspace_bytes(None) == 0
    assert "NULL" in L.md2_last_error().decode()
    d = desc()
    x = ctypes.c_void_p(256)
    for args in [(None, None, x, x, x), (x, None, None, x, x), (x, None, x, None, x), (x, None, x, x, None)]:
        assert L.md2_depth_eval(ctypes.byref(d), *args, None) == -1
        assert "NULL" in L.md2_last_error().decode()


def test_post_process_needs_the_flipped_pass(L):
    d = desc(post_process=True)
    x = ctypes.c_void_p(256)
    assert L.md2_depth_eval(ctypes.byref(d), x, None, x, x, x, None) == -1
    assert "disp_flipped" in L.md2_last_error().decode()


def test_workspace_is_monotone_in_ground_truth_pixels(L):
    sizes = []
    for B, GH, GW in [(1, 1, 1), (1, 13, 41), (1, 37, 124), (3, 37, 124), (2, 375, 1242), (16, 375, 1242)]:
        d = desc(batch=B, gt_height=GH, gt_width=GW, crop=None)
        ws = L.md2_depth_eval_workspace_bytes(ctypes.byref(d))
        assert ws % 256 == 0 and ws >= 4 * B * GH * GW   # the fp32 prediction plane
        sizes.append((B * GH * GW, ws))
    assert all(a[1] <= b[1] for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[0][1] < sizes[-1][1]
    # one pooled population needs no more than one per image
    pooled = L.md2_depth_eval_workspace_bytes(ctypes.byref(desc(pool_batch=True)))
    assert pooled <= L.md2_depth_eval_workspace_bytes(ctypes.byref(desc(pool_batch=False)))


def test_flag_defaults_follow_the_reference():
    e, m = desc(), desc(mode="monitor")
    assert e.flags == _lib.EVAL_GT_RANGE | _lib.EVAL_MEDIAN_SCALE
    assert m.flags == (_lib.EVAL_RESIZE_DEPTH | _lib.EVAL_MEDIAN_SCALE | _lib.EVAL_MEDIAN_LOWER
                       | _lib.EVAL_POOL_BATCH)
    assert desc(crop=None).flags == _lib.EVAL_MEDIAN_SCALE   # evaluate_depth.py:199-200: gt > 0, no crop
    with pytest.raises(ValueError):
        desc(mode="other")


def test_depth_metrics_has_no_cpu_fallback():
    from monodepth2_amd.eval_ops import depth_metrics
    with pytest.raises(RuntimeError, match="GPU only"):
        depth_metrics(torch.rand(1, 1, 8, 8), torch.rand(1, 9, 9))


def test_restatement_reproduces_the_reference_golden():
    """The fp64 restatement of compute_depth_losses against the reference's own fp32 run.
    Bar: the golden is an fp32 run, so it carries the roundings of the median element, of
    the ratio and of the fp32 mean (2^-24 = 6e-8 each), the ratio's amplified by the
    metric's sensitivity to a common scale (below 2 here): 5e-7 relative covers that and
    is far below what a changed formula gives (the other median convention on this even
    count moves the ratio by 1e-5); the threshold fractions are counts over the same
    n (their pixels near 1.25^k were removed), exact up to the fp32 mean: 2 ulp."""
    sig, gt, golden = eval_case.load_golden()
    assert gt.shape == (2, 375, 1242) and sig.shape == (2, 1, 24, 80)
    e64 = eval_case.evaluate_np(sig, gt, np.float64, mode="monitor")[0]
    rel = np.abs(e64[:7] - golden) / np.abs(golden)
    print("restatement vs golden, relative:", rel)
    assert (rel[:4] < 5e-7).all(), rel
    assert (rel[4:] < 2.4e-7).all(), rel
    assert e64[8] == np.count_nonzero(gt[:, 153:371, 44:1197])


@pytest.mark.parametrize("argv,what", [
    (["--eval_mono"], "data_path"),
    (["--eval_mono", "--eval_split", "benchmark", "--ext_disp_to_eval", "x.npy"], "benchmark"),
    (["--eval_mono", "--eval_eigen_to_benchmark", "--ext_disp_to_eval", "x.npy"], "eigen_to_benchmark"),
])
def test_out_of_scope_paths_are_refused_clearly(argv, what):
    from monodepth2_amd.evaluate_depth import evaluate
    from monodepth2_amd.options import MonodepthOptions
    with pytest.raises(NotImplementedError, match=what):
        evaluate(MonodepthOptions().parse(argv))


def test_mono_or_stereo_must_be_chosen():
    from monodepth2_amd.evaluate_depth import evaluate
    from monodepth2_amd.options import MonodepthOptions
    for argv in ([], ["--eval_mono", "--eval_stereo"]):
        with pytest.raises(SystemExit, match="mono or stereo"):
            evaluate(MonodepthOptions().parse(argv))
