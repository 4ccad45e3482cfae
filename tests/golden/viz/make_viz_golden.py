"""Makes tests/golden/viz/viz.npz on the CPU:  python tests/golden/viz/make_viz_golden.py

The reference's test_simple.py cannot run here (it imports torchvision and downloads its
model), so the golden is captured from the libraries its lines 136-155 call, through their
public APIs, one image at a time as the reference does:

    136-137  torch.nn.functional.interpolate(disp, (H, W), mode="bilinear", align_corners=False)
    151-152  np.percentile(resized, percentile) of the squeezed fp32 array
    153      matplotlib.colors.Normalize(vmin=resized.min(), vmax=that percentile)
    154-155  matplotlib.cm.ScalarMappable(norm, "magma").to_rgba(resized)[:, :, :3] * 255 as uint8

Recorded: the library versions, the magma table as bytes, and per case of
tests/viz_case.build_cases() the input, torch-CPU's resized map, vmin, vmax and the bytes;
per resize case also the bilinear formula in fp64 with fp64 source coordinates and the
floor max |torch CPU - fp64|.  Before anything is written the numpy restatement of
tests/viz_case.py is measured against all of it (and on a batch of random maps, and on one
KITTI-sized resize); the counts it prints are the ones DESIGN §6e quotes.
"""
import os
import sys
import warnings

import matplotlib
import matplotlib.cm
import matplotlib.colors
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import viz_case as vc  # noqa: E402


def library_picture(resized, percentile):
    """test_simple.py:151-155 for one resized map (H, W) fp32."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # a NaN map: numpy warns, the result is nan
        vmax = np.percentile(resized, percentile)
        vmin = resized.min()
        norm = matplotlib.colors.Normalize(vmin=vmin, vmax=vmax)
        mapper = matplotlib.cm.ScalarMappable(norm=norm, cmap="magma")
        rgb = (mapper.to_rgba(resized)[:, :, :3] * 255).astype(np.uint8)
    return np.float32(vmin), np.float32(vmax), rgb


def library_resize(disp, size):
    """test_simple.py:136-137 on the CPU; disp (B,1,h,w) -> (B,H,W)."""
    out = torch.nn.functional.interpolate(torch.from_numpy(disp), size, mode="bilinear", align_corners=False)
    return out[:, 0].numpy()


def resize_f64(disp, size):
    """The bilinear formula in fp64 with fp64 source coordinates; disp (B,1,h,w) -> (B,H,W)."""
    d = disp[:, 0].astype(np.float64)

    def coords(out, inp):
        src = np.maximum((inp / out) * (np.arange(out, dtype=np.float64) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), inp - 1)
        return i0, np.minimum(i0 + 1, inp - 1), src - i0

    y0, y1, fy = coords(size[0], d.shape[1])
    x0, x1, fx = coords(size[1], d.shape[2])
    top = (1 - fx) * d[:, y0][:, :, x0] + fx * d[:, y0][:, :, x1]
    bot = (1 - fx) * d[:, y1][:, :, x0] + fx * d[:, y1][:, :, x1]
    return (1 - fy)[:, None] * top + fy[:, None] * bot


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or (np.isnan(a).all() and np.isnan(b).all())


def main():
    lut = (matplotlib.colormaps["magma"](np.arange(256))[:, :3] * 255).astype(np.uint8)
    assert len({tuple(row) for row in lut}) == 256          # viz_case.lut_index inverts it
    print("magma table, packed R | G << 8 | B << 16:")
    packed = lut[:, 0].astype(np.uint32) | lut[:, 1].astype(np.uint32) << 8 | lut[:, 2].astype(np.uint32) << 16
    for i in range(0, 256, 8):
        print("    " + ", ".join("0x%06x" % v for v in packed[i:i + 8]) + ",")

    out = {"lut": lut, "versions": np.array(["numpy " + np.__version__, "matplotlib " + matplotlib.__version__,
                                             "torch " + torch.__version__])}
    names = []
    for name, (disp, size, pct) in vc.build_cases().items():
        names.append(name)
        resized = library_resize(disp, size)
        pictures = [library_picture(r, pct) for r in resized]
        vmin = np.array([p[0] for p in pictures], np.float32)
        vmax = np.array([p[1] for p in pictures], np.float32)
        rgb = np.stack([p[2] for p in pictures])
        out.update({"in_" + name: disp, "size_" + name: np.array(size, np.int32), "pct_" + name: np.int32(pct),
                    "resized_" + name: resized, "vmin_" + name: vmin, "vmax_" + name: vmax, "rgb_" + name: rgb})
        my_rgb, my_resized, my_stats = vc.colorize_np(disp, size, pct, lut)
        if name.startswith("e_"):
            # the identity resize returns the input; the later stages are exact
            assert np.array_equal(resized, disp[:, 0], equal_nan=True), name
            assert same_bits(my_stats[:, 0], vmin) and same_bits(my_stats[:, 1], vmax), (name, my_stats, vmin, vmax)
            assert np.array_equal(my_rgb, rgb), name
            print("%-20s exact: vmin, vmax bit-equal, %d bytes equal" % (name, rgb.size))
        else:
            f64 = resize_f64(disp, size)
            floor = float(np.abs(resized.astype(np.float64) - f64).max())
            mine = float(np.abs(my_resized.astype(np.float64) - f64).max())
            out.update({"f64_" + name: f64, "floor_" + name: np.float64(floor)})
            a, b = vc.lut_index(rgb, lut), vc.lut_index(my_rgb, lut)
            diff = a != b
            assert np.abs(a - b).max() <= 1 and diff.mean() <= 0.005, name
            assert mine <= 4 * floor, (name, mine, floor)
            print("%-20s floor |torch - fp64| %.3e, restatement %.3e (%.2f floors), max |restatement - torch| "
                  "%.3e, pixels off the library's bytes: %d of %d" %
                  (name, floor, mine, mine / floor, float(np.abs(my_resized - resized).max()), int(diff.sum()), diff.size))
    out["names"] = np.array(names)

    # the later stages against the libraries on random maps of many kinds (not recorded)
    rng = np.random.RandomState(99)
    maps = pixels = 0
    for i in range(120):
        h, w = int(rng.randint(1, 90)), int(rng.randint(1, 200))
        kind = i % 4
        m = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
        if kind == 1:
            m = (np.round(m * 20) / 20).astype(np.float32)                      # heavy in ties
        elif kind == 2:
            m = rng.normal(0.0, 3.0, (h, w)).astype(np.float32)                 # signed
        elif kind == 3:
            m = vc.sigmoid_map(h, w, i)
        pct = int(rng.choice([95, 95, 95, 0, 50, 100, 7, 33, 99]))
        vmin, vmax, rgb = library_picture(m, pct)
        my_rgb, _, my_stats = vc.colorize_np(m[None], None, pct, lut)
        assert same_bits(my_stats[0, 0], vmin) and same_bits(my_stats[0, 1], vmax), (i, h, w, pct)
        assert np.array_equal(my_rgb[0], rgb), (i, h, w, pct)
        maps, pixels = maps + 1, pixels + h * w
    print("later stages: %d random maps, %d pixels, vmin/vmax bit-equal and every byte equal" % (maps, pixels))

    # a KITTI-sized resize (not recorded): 192 x 640 -> 375 x 1242
    disp = vc.sigmoid_map(192, 640, 77)[None, None]
    resized = library_resize(disp, (375, 1242))
    _, _, rgb = library_picture(resized[0], 95)
    my_rgb, my_resized, _ = vc.colorize_np(disp, (375, 1242), 95, lut)
    a, b = vc.lut_index(rgb, lut), vc.lut_index(my_rgb[0], lut)
    f64 = resize_f64(disp, (375, 1242))
    print("192x640 -> 375x1242: floor %.3e, restatement %.3e, max rel |restatement - torch| %.3e, pixels off: "
          "%d of %d (largest index step %d)" %
          (float(np.abs(resized - f64).max()), float(np.abs(my_resized - f64).max()),
           float((np.abs(my_resized - resized) / resized).max()), int((a != b).sum()), a.size, int(np.abs(a - b).max())))
    out["big_mismatch"] = np.array([int((a != b).sum()), a.size], np.int64)

    path = os.path.join(HERE, "viz.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
