"""Makes tests/golden/logpanel/logpanel.npz and warp_<case>_<frame>.npz on the CPU:

    python tests/golden/logpanel/make_logpanel_golden.py --ref <checkout of the reference>

Run where the reference is at hand (it never travels to the GPU machine).  Recorded:

  * per case of tests/logpanel_case.disp_cases(): the input, the result of the reference's
    own utils.normalize_image on it (torch on the CPU), its minimum and maximum, and the
    bytes the image writer makes of that result.  Before anything is written the numpy
    restatement (logpanel_case.normalize / stats / quantise) must equal all of it bit for bit;
  * for full_mono_b2_192x640 and full_stereo_b2_192x640 (tests/golden/make_golden.py's
    cases, whose fixtures hold checksums only): the reference's warped source frames of
    scale 0, outputs[("color", f, 0)], from its generate_images_pred on the CPU, as the
    writer's bytes, and per byte whether golden * 255 lies within 255 * 2e-5 of an integer
    (bit-packed), one file per case and frame — the only places where an fp32 warp that is within 2e-5 of the
    reference's (the bar of test_hip_matches_reference) may land on the neighbouring byte.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/golden: make_golden
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # tests: logpanel_case
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))   # the package

import logpanel_case as lc                                    # noqa: E402
from make_golden import CASES, import_reference, run_case     # noqa: E402

WARP_CASES = ["full_mono_b2_192x640", "full_stereo_b2_192x640"]
WARP_ATOL = 2e-5   # test_hip_matches_reference's bar on the fp32 warps


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)]) and \
        np.array_equal(np.isnan(a), np.isnan(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (utils.py, trainer.py, layers.py)")
    args = ap.parse_args()
    ref_trainer, ref_layers = import_reference(args.ref)
    from utils import normalize_image   # the reference's, utils.py:22-28

    out = {"versions": np.array(["numpy " + np.__version__, "torch " + torch.__version__])}
    names = []
    for name, x in lc.disp_cases().items():
        names.append(name)
        ref = normalize_image(torch.from_numpy(x.copy())).numpy()
        mi, ma = np.float32(torch.from_numpy(x).min().item()), np.float32(torch.from_numpy(x).max().item())
        assert ref.dtype == np.float32
        my_mi, my_ma = lc.stats(x)
        mine = lc.normalize(x)
        assert same(my_mi, mi) and same(my_ma, ma), (name, my_mi, mi, my_ma, ma)
        assert same(mine, ref), (name, int((mine.view(np.uint32) != ref.view(np.uint32)).sum()))
        recip = ((x - mi) * (np.float32(1.0) / (np.float32(np.float64(ma) - np.float64(mi)) if ma != mi
                                                 else np.float32(1e5)))).astype(np.float32)
        with np.errstate(invalid="ignore"):
            print("%-12s %s bit-equal to normalize_image; a reciprocal multiply would change %d of %d values, "
                  "%d bytes" % (name, x.shape, int((recip != ref).sum() - np.isnan(ref).sum()), x.size,
                                int((lc.quantise(recip) != lc.quantise(ref)).sum())))
        out.update({"in_" + name: x, "norm_" + name: ref, "stats_" + name: np.array([mi, ma], np.float32),
                    "bytes_" + name: lc.quantise(ref)})
    out["names"] = np.array(names)

    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(lc.quantise(k), np.arange(256, dtype=np.uint8))
    assert np.array_equal((torch.from_numpy(k) * 255).clamp(0, 255).to(torch.uint8).numpy(), np.arange(256))

    for name in WARP_CASES:
        spec = CASES[name]
        spec = tuple(spec[:6]) + (True,)   # keep the full planes
        rec = run_case(ref_trainer, ref_layers, name, spec)
        for f in spec[3][1:]:
            w = rec["warp_{}_0".format(f)]
            p = w.astype(np.float64) * 255.0
            near = np.abs(p - np.rint(p)) <= 255.0 * WARP_ATOL
            wp = os.path.join(HERE, "warp_{}_{}.npz".format(name, f))
            np.savez_compressed(wp, q=lc.quantise(w), near=np.packbits(near.reshape(-1)))
            print("%s frame %s: %s, %d of %d bytes within %.1e of a step; %d bytes on disk" %
                  (name, f, w.shape, int(near.sum()), near.size, 255.0 * WARP_ATOL, os.path.getsize(wp)))

    path = os.path.join(HERE, "logpanel.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
