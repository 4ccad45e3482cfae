"""md2_png_encode (csrc/pngenc.hip) against the restatement of its format rules
(tests/png_encode_case.py), byte for byte, on every named case; the files back
through our own decoder; the capacity refusal; the two writers and the evaluation command with
--device_png_encode against their Pillow routes, pixel for pixel."""
import io
import types

import numpy as np
import pytest
import torch
from PIL import Image

import png_encode_case as ec

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = ec.cases()
_want = {}


def want(name):
    """The restatement's files of a case, computed once."""
    if name not in _want:
        _want[name] = [ec.encode_np(f, k, s) for f, k, s in CASES[name]]
    return _want[name]


def device_frames(name):
    return [torch.from_numpy(np.ascontiguousarray(np.asarray(f).view(np.int16) if k == ec.GRAY16 else f)).to(DEV)
            for f, k, _ in CASES[name]]


@pytest.mark.parametrize("name", list(CASES))
def test_bytes_equal_the_restatement(name):
    from monodepth2_amd import png_ops
    got = png_ops.encode_png_batch(device_frames(name), kind=[k for _, k, _ in CASES[name]],
                                   segment_bytes=[s for _, _, s in CASES[name]], check=True)
    assert len(got) == len(want(name))
    for i, (g, w) in enumerate(zip(got, want(name))):
        assert len(g) == len(w), (name, i, len(g), len(w))
        assert g == w, (name, i, next(k for k in range(len(w)) if g[k] != w[k]))


def test_kinds_are_told_from_the_tensors_and_a_stacked_tensor_is_taken_where_it_lies():
    from monodepth2_amd import png_ops
    assert png_ops.encode_png_batch(device_frames("mixed_batch")[:2], segment_bytes=[1024, 4096]) == \
        want("mixed_batch")[:2]
    frame = CASES["panel_like_48x160_rgb"][0][0]
    stack = torch.from_numpy(np.stack([frame, frame[::-1].copy()])).to(DEV)
    got = png_ops.encode_png_batch(stack)
    assert got[0] == want("panel_like_48x160_rgb")[0] and got[1] == ec.encode_np(frame[::-1].copy(), ec.RGB8)
    assert png_ops.encode_png_batch(stack) == got                          # repeatable


def test_rgb_files_decode_through_our_own_decoder():
    from monodepth2_amd import png_ops
    names = [n for n in CASES if n != "mixed_batch" and CASES[n][0][1] == ec.RGB8]
    files = [want(n)[0] for n in names]
    streams = [png_ops.parse_png(f) for f in files]
    assert all(s is not None for s in streams)
    flat, offsets, sizes = png_ops.decode_png_frames(streams, DEV, names)       # raises on a status that is not 0
    host = flat.cpu().numpy()
    for n, o, (h, w) in zip(names, offsets, sizes):
        assert np.array_equal(host[o:o + h * w * 3].reshape(h, w, 3), CASES[n][0][0]), n


def test_a_capacity_that_is_too_small():
    from monodepth2_amd import _lib, png_ops
    frames = device_frames("mixed_batch")[:3]
    specs = CASES["mixed_batch"][:3]
    geos = [(f.shape[0], f.shape[1], k, s) for f, k, s in specs]
    need = [len(ec.encode_info(f, k, s)["zstream"]) for f, k, s in specs]
    sizes = [f.numel() * f.element_size() for f in frames]
    offsets = [0, 4096 * 4, 4096 * 8]
    flat = torch.zeros(4096 * 9, dtype=torch.uint8, device=DEV)
    for f, o, b in zip(frames, offsets, sizes):
        flat[o:o + b] = f.contiguous().view(torch.uint8).reshape(-1)
    caps = [need[0], need[1] - 1, need[2]]
    images, out_bytes, ws_bytes = png_ops.describe_png_encode(geos, offsets, caps)
    png_ops.check_png_encode_described(images, 3, flat.numel(), out_bytes)
    out = torch.full((out_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
    lengths, status = png_ops.run_png_encode(flat, images, 3, out, ws_bytes, torch.device(DEV, 0))
    assert status.cpu().tolist() == [0, _lib.PNGENC_ST_SPACE, 0]
    assert lengths.cpu().tolist() == need
    host = out.cpu().numpy()
    for i in (0, 2):
        o = images[i].out_offset
        assert host[o:o + need[i]].tobytes() == ec.encode_info(*specs[i])["zstream"]
    o = images[1].out_offset
    assert (host[o:images[2].out_offset] == 0xA5).all()                     # nothing of its own range
    assert (host[images[0].out_offset + need[0]:o] == 0xA5).all()
    assert (host[images[2].out_offset + need[2]:] == 0xA5).all()


def test_write_benchmark_pngs_on_the_device(tmp_path):
    from monodepth2_amd.eval_ops import write_benchmark_pngs
    rng = np.random.default_rng(5)
    maps = (np.linspace(300, 20480, 40 * 70).reshape(1, 40, 70) + rng.integers(0, 40000, (3, 1, 1))).astype(np.uint16)
    maps[2, :5] = 65535
    t = torch.from_numpy(maps.view(np.int16)).to(DEV)
    paths = write_benchmark_pngs(t, str(tmp_path / "dev"), start=7, device_encode=True)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["{:010d}.png".format(7 + i) for i in range(3)]
    for p, a in zip(paths, maps):
        im = Image.open(p)
        assert im.mode in ("I;16", "I;16B", "I") and np.array_equal(np.asarray(im).astype(np.uint16), a)
        assert open(p, "rb").read() == ec.encode_np(a, ec.GRAY16)
    with pytest.raises(RuntimeError, match="GPU only"):
        write_benchmark_pngs(maps, str(tmp_path / "dev"), device_encode=True)


def test_write_panel_on_the_device(tmp_path):
    from monodepth2_amd.log_ops import write_panel
    sheet = np.stack([CASES["panel_like_48x160_rgb"][0][0], CASES["panel_like_48x160_rgb"][0][0][:, ::-1].copy()])
    panel = types.SimpleNamespace(sheet=torch.from_numpy(sheet).to(DEV), layout=(48, 160, {"color_0_0/0": (0, 0, 24, 80)}))
    dev = write_panel(panel, str(tmp_path / "dev"), 12, device_encode=True)
    pil = write_panel(panel, str(tmp_path / "pil"), 12)
    assert [p.rsplit("/", 1)[1] for p in dev] == [p.rsplit("/", 1)[1] for p in pil] == \
        ["step_0000012_0.png", "step_0000012_1.png"]
    for d, p, a in zip(dev, pil, sheet):
        assert np.array_equal(np.asarray(Image.open(d).convert("RGB")), a)
        assert np.array_equal(np.asarray(Image.open(p)), a)
    assert (tmp_path / "dev" / "layout.json").read_text() == (tmp_path / "pil" / "layout.json").read_text()


def test_evaluate_depth_benchmark_with_the_flag(tmp_path):
    from monodepth2_amd.evaluate_depth import evaluate
    from monodepth2_amd.options import MonodepthOptions
    rng = np.random.default_rng(9)
    disp = (0.02 + 0.5 * rng.random((4, 6, 20))).astype(np.float32)
    np.save(tmp_path / "disps.npy", disp)
    runs = {}
    for name, flag in (("pil", []), ("dev", ["--device_png_encode"])):
        argv = ["--eval_mono", "--eval_split", "benchmark", "--ext_disp_to_eval", str(tmp_path / "disps.npy"),
                "--eval_out_dir", str(tmp_path / name)] + flag
        runs[name] = evaluate(MonodepthOptions().parse(argv))
    assert len(runs["pil"]) == len(runs["dev"]) == 4
    for a, b in zip(runs["pil"], runs["dev"]):
        assert a.rsplit("/", 1)[1] == b.rsplit("/", 1)[1]
        x, y = Image.open(a), Image.open(b)
        assert x.size == y.size == (1216, 352)
        assert np.array_equal(np.asarray(x), np.asarray(y))
        assert open(a, "rb").read() != open(b, "rb").read()
