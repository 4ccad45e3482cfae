"""Shared by tests/test_export16_*.py: a numpy restatement of the reference's benchmark
export (evaluate_depth.py:148-163: cv2.resize of the scaled disparity to 1216 x 352,
5.4 / disp, clip to [0, 80], uint16(depth * 256)) in a chosen precision, the inputs the
tests run it on, and the comparison rule.

`export16_np` is built from tests/eval_case.py's `scaled_disp` (torch's fp32 product and
sum), `post_process` and `resize` (half-pixel bilinear), in `dt` after disp_to_depth:
dt=float64 is the yardstick, dt=float32 the formulation a host loop in fp32 would run.
cv2 itself is not available to these tests: what is pinned is the written formula.

The three cases numpy's float-to-integer cast leaves undefined are defined as the kernel
defines them: a resized disparity of exactly 0 gives clip_max * quant, a negative one
gives 0, NaN gives 0.

Truncation is discontinuous, so where the fp64 value x = depth * quant lies within DELTA of
an integer a correct evaluation in another order may land one count away; everywhere else
equality is exact.  DELTA = 1e-6 is far above fp64 reordering error (~1e-11 at 20480
counts) and far below the fp32 formulation's own 0.05 counts.
"""
import numpy as np

import eval_case as ec

DELTA = 1e-6
MAX_EXCLUDED = 1e-4      # share of the unclipped pixels that may sit within DELTA of an integer
CLIP_MARGIN = 1e-9       # depth >= clip_max * (1 + CLIP_MARGIN) before the clip: exactly clip_max * quant


def export16_values(sig, sig_flipped, out_hw, dt, scale_factor=5.4, clip_max=80.0, quant=256.0, min_depth=0.1,
                    max_depth=100.0):
    """-> (x, depth): x (B,OH,OW) the `dt` values depth * quant before the cast, with the
    three edge cases resolved, and the depth before the clip."""
    sd = ec.scaled_disp(sig[:, 0], min_depth, max_depth)
    if sig_flipped is not None:
        sd = ec.post_process(sd, ec.scaled_disp(sig_flipped[:, 0], min_depth, max_depth)[:, :, ::-1], dt)
    r = ec.resize(sd.astype(dt), out_hw[0], out_hw[1], dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = dt(scale_factor) / r
    clipped = np.clip(depth, dt(0), dt(clip_max))
    clipped = np.where(np.isnan(clipped), dt(0), clipped)            # NaN -> 0 (r == 0 -> inf -> clip_max, r < 0 -> 0)
    return clipped * dt(quant), depth


def export16_np(sig, sig_flipped, out_hw, dt, **kw):
    """The (B,OH,OW) uint16 maps of sigmoid disparities `sig` (B,1,h,w) in precision `dt`."""
    return export16_values(sig, sig_flipped, out_hw, dt, **kw)[0].astype(np.uint16)


def straddling_inputs():
    """eval_case.make_inputs(B=3, h=24, w=80, seed=7) with image 1 (and its flipped pass)
    scaled by float32(0.012), so that its depths straddle the 80 m clip."""
    sig, sigf, _ = ec.make_inputs(B=3, h=24, w=80, seed=7)
    sig, sigf = sig.copy(), sigf.copy()
    sig[1] *= np.float32(0.012)
    sigf[1] *= np.float32(0.012)
    return sig, sigf


def smooth_inputs(B, h, w, seed):
    """Sigmoid disparities of any size (eval_case.make_inputs needs h, w >= 1 as well), the
    middle image scaled to straddle the clip when there are at least two."""
    sig, sigf, _ = ec.make_inputs(B=B, h=h, w=w, GH=2, GW=2, seed=seed)
    sig, sigf = sig.copy(), sigf.copy()
    if B >= 2:
        sig[B // 2] *= np.float32(0.012)
        sigf[B // 2] *= np.float32(0.012)
    return sig, sigf


def compare(got, sig, sig_flipped, out_hw, **kw):
    """The rule of the GPU tests: `got` (B,OH,OW) uint16 against the fp64 restatement.
    -> dict of figures; raises AssertionError where the rule is broken."""
    x, depth = export16_values(sig, sig_flipped, out_hw, np.float64, **kw)
    want = x.astype(np.uint16)
    clip_max, quant = kw.get("clip_max", 80.0), kw.get("quant", 256.0)
    surely_clipped = depth >= clip_max * (1 + CLIP_MARGIN)
    unclipped = depth < clip_max
    near = np.abs(x - np.rint(x)) <= DELTA
    diff = got.astype(np.int64) - want.astype(np.int64)
    figures = dict(pixels=int(x.size), near=int((near & unclipped).sum()), unclipped=int(unclipped.sum()),
                   clipped=int(surely_clipped.sum()), differ=int((diff != 0).sum()),
                   max_diff=int(np.abs(diff).max()))
    print("export16", tuple(sig.shape), "->", tuple(out_hw), "pp" if sig_flipped is not None else "plain", figures)
    assert got.shape == want.shape and got.dtype == np.uint16
    assert (got[surely_clipped] == int(clip_max * quant)).all()
    assert (diff[~near] == 0).all(), figures
    assert (np.abs(diff[near]) <= 1).all(), figures
    assert (near & unclipped).sum() <= MAX_EXCLUDED * max(int(unclipped.sum()), 1), figures
    return figures
