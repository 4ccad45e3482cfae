"""CPU-side checks of the PNG encoder's ABI (md2_png_encode, csrc/pngenc.hip), in the manner
of test_jpeg_encode_abi.py: struct layout, exports, the capacity bound, the workspace size,
every refusal with its message, the GPU-only error of encode_png_batch, png_file_bytes and the
--device_png_encode flag — no kernel is launched."""
import ctypes
import io

import numpy as np
import pytest
import torch

from monodepth2_amd import _lib, png_ops
from monodepth2_amd.build import build

import png_encode_case as ec

NAMES = {"md2_png_encode_bound", "md2_png_encode_workspace_bytes", "md2_png_encode_check", "md2_png_encode"}
RGB8, GRAY16 = _lib.PNGENC_RGB8, _lib.PNGENC_GRAY16


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def image(h, w, kind=RGB8, s=16384, in_offset=0, out_offset=0, ws_offset=0, cap=None, reserved=0):
    im = _lib.PngEncImage()
    im.height, im.width, im.kind, im.segment_bytes = h, w, kind, s
    im.in_offset, im.out_offset, im.ws_offset, im.reserved = in_offset, out_offset, ws_offset, reserved
    im.out_capacity = 1 << 20 if cap is None else cap
    return im


def batch(*ims):
    return (_lib.PngEncImage * len(ims))(*ims)


def check(L, ims, in_bytes=1 << 30, out_bytes=1 << 30):
    return L.md2_png_encode_check(ims, len(ims), in_bytes, out_bytes)


def refused(L, rc, text):
    assert rc == -1
    assert text in L.md2_last_error().decode(), L.md2_last_error().decode()


def test_exports_and_abi(L):
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert NAMES <= set(_lib.EXPORTS)
    for n in NAMES:
        assert hasattr(L, n), n
    assert ctypes.sizeof(_lib.PngEncImage) == 48
    offs = {f: getattr(_lib.PngEncImage, f).offset for f, _ in _lib.PngEncImage._fields_}
    assert offs == dict(in_offset=0, out_offset=8, ws_offset=16, out_capacity=24, height=28, width=32, kind=36,
                        segment_bytes=40, reserved=44)
    assert (_lib.PNGENC_RGB8, _lib.PNGENC_GRAY16, _lib.PNGENC_ST_SPACE) == (0, 1, 1)
    assert (png_ops.KIND_RGB8, png_ops.KIND_GRAY16) == (ec.RGB8, ec.GRAY16)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (40, 70), (352, 1216), (8192, 8192)])
@pytest.mark.parametrize("kind", [RGB8, GRAY16])
@pytest.mark.parametrize("s", [1024, 16384, 32768])
def test_bound_is_all_stored_plus_flushes(L, h, w, kind, s):
    total = h * (1 + (3 if kind == RGB8 else 2) * w)
    want = total + 10 * -(-total // s) + 6
    assert L.md2_png_encode_bound(h, w, kind, s) == want == ec.encode_bound(h, w, kind, s)
    assert png_ops.encode_bound(h, w, kind, s) == want


@pytest.mark.parametrize("h,w,kind,s,text", [(0, 8, 0, 1024, "1..8192"), (8, 0, 0, 1024, "1..8192"),
                                             (8193, 8, 1, 1024, "1..8192"), (8, 8193, 0, 1024, "1..8192"),
                                             (8, 8, 2, 1024, "unknown kind"), (8, 8, -1, 1024, "unknown kind"),
                                             (8, 8, 0, 512, "power of two"), (8, 8, 0, 65536, "power of two"),
                                             (8, 8, 1, 3000, "power of two")])
def test_a_bad_geometry_is_refused_everywhere(L, h, w, kind, s, text):
    assert L.md2_png_encode_bound(h, w, kind, s) == 0
    assert text in L.md2_last_error().decode()
    assert L.md2_png_encode_workspace_bytes(batch(image(8, 8), image(h, w, kind, s)), 2) == 0
    assert text in L.md2_last_error().decode()
    refused(L, check(L, batch(image(h, w, kind, s))), text)
    with pytest.raises((RuntimeError, ValueError)):
        png_ops.encode_bound(h, w, kind, s)


def test_workspace_holds_scanlines_row_sums_tokens_and_scratch(L):
    ims = batch(image(352, 1216, GRAY16), image(17, 33, RGB8, 1024))
    need = L.md2_png_encode_workspace_bytes(ims, 2)
    each = [L.md2_png_encode_workspace_bytes(batch(im), 1) for im in ims]
    assert need == sum(each) and all(e % 256 == 0 for e in each)
    for (h, w, bpp, s), e in zip([(352, 1216, 2, 16384), (17, 33, 3, 1024)], each):
        total = h * (1 + bpp * w)
        nseg = -(-total // s)
        floor = total + 16 * h + 4 * total + nseg * (s + 16) + 8 * nseg
        assert floor <= e <= floor + 16 * 4 + 256
    assert L.md2_png_encode_workspace_bytes(ims, 0) == 0 and "1..4096" in L.md2_last_error().decode()
    assert L.md2_png_encode_workspace_bytes(None, 1) == 0 and "NULL" in L.md2_last_error().decode()


def test_a_good_batch_passes_and_the_last_byte_counts(L):
    a = image(16, 16, RGB8, 1024, 0, 0, 0, cap=100)
    wa = L.md2_png_encode_workspace_bytes(batch(a), 1)
    b = image(37, 53, GRAY16, 4096, 768, 101, wa, cap=1000)
    ims = batch(a, b)
    in_end, out_end = 768 + 37 * 53 * 2, 101 + 1000
    assert check(L, ims, in_bytes=in_end, out_bytes=out_end) == 0
    refused(L, check(L, ims, in_bytes=in_end - 1, out_bytes=out_end), "frame reaches past in_bytes")
    refused(L, check(L, ims, in_bytes=in_end, out_bytes=out_end - 1), "output range reaches past out_bytes")
    refused(L, check(L, batch(image(8, 8, in_offset=1 << 40))), "frame reaches past in_bytes")
    refused(L, check(L, batch(image(8, 8, out_offset=1 << 40))), "output range reaches past out_bytes")
    assert check(L, batch(image(8, 8, cap=0)), out_bytes=0) == 0   # nothing fits: ST_SPACE at run time
    refused(L, check(L, batch(a, image(37, 53, GRAY16, 4096, 769, 101, wa))), "multiple of 2")
    assert check(L, batch(image(8, 8, RGB8, in_offset=1))) == 0     # 8-bit frames are tight: any byte offset
    refused(L, check(L, batch(a, image(37, 53, GRAY16, 4096, 768, 101, wa + 256))), "ws_offset")
    refused(L, check(L, batch(image(8, 8, ws_offset=256))), "ws_offset")
    refused(L, check(L, batch(image(8, 8, reserved=1))), "reserved")
    refused(L, L.md2_png_encode_check(None, 1, 1 << 20, 1 << 20), "NULL")
    refused(L, L.md2_png_encode_check(batch(image(8, 8)), 4097, 1 << 20, 1 << 20), "1..4096")
    refused(L, L.md2_png_encode_check(batch(image(8, 8)), 0, 1 << 20, 1 << 20), "1..4096")


def run(L, ims, workspace_bytes=1 << 30, **kw):
    """md2_png_encode on addresses that must never be dereferenced."""
    args = dict(inp=4096, dev=4096, ws=4096, out=4096, sb=4096, st=4096)
    args.update(kw)
    return L.md2_png_encode(args["inp"], 1 << 24, ims, args["dev"], len(ims), args["ws"], workspace_bytes,
                            args["out"], 1 << 24, args["sb"], args["st"], None)


def test_encode_refuses_before_it_launches(L):
    a = image(16, 16, RGB8, 1024)
    ims = batch(a, image(8, 8, GRAY16, 1024, 768, 1 << 20, L.md2_png_encode_workspace_bytes(batch(a), 1)))
    for name in ("inp", "dev", "ws", "out", "sb", "st"):
        refused(L, run(L, ims, **{name: None}), "NULL")
    refused(L, run(L, ims, inp=4097), "aligned")
    refused(L, run(L, ims, ws=4096 + 128), "aligned")
    refused(L, run(L, ims, dev=4100), "aligned")
    refused(L, run(L, ims, workspace_bytes=L.md2_png_encode_workspace_bytes(ims, 2) - 1), "more workspace")
    refused(L, run(L, batch(image(16, 16, 5))), "unknown kind")
    refused(L, run(L, batch(image(16, 16, RGB8, 2048, ws_offset=512))), "ws_offset")


def test_describe_lays_out_ranges_and_running_sums(L):
    geos = [(16, 16, RGB8, 1024), (37, 53, GRAY16, 4096), (1, 1, RGB8, 16384)]
    images, out_bytes, ws_bytes = png_ops.describe_png_encode(geos, [0, 768, 768 + 37 * 53 * 2])
    assert ws_bytes == L.md2_png_encode_workspace_bytes(images, 3)
    pos = 0
    for im, g in zip(images, geos):
        assert im.out_offset == pos and im.out_capacity == ec.encode_bound(*g)
        pos += (im.out_capacity + 15) // 16 * 16
    assert out_bytes == pos
    png_ops.check_png_encode_described(images, 3, 768 + 37 * 53 * 2 + 3, out_bytes)
    with pytest.raises(RuntimeError, match="in_bytes"):
        png_ops.check_png_encode_described(images, 3, 768 + 37 * 53 * 2 + 2, out_bytes)


def test_wrapper_is_gpu_only():
    with pytest.raises(RuntimeError, match="GPU only"):
        png_ops.encode_png_batch([], device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        png_ops.encode_png_batch([torch.zeros(4, 4, 3, dtype=torch.uint8)], device="cpu")
    from monodepth2_amd import eval_ops
    with pytest.raises(RuntimeError, match="GPU only"):
        eval_ops.write_benchmark_pngs(torch.zeros(1, 4, 4, dtype=torch.int16), "/nonexistent", device_encode=True)


def test_png_file_bytes_wraps_a_zlib_stream_like_the_restatement():
    from PIL import Image
    for name in ("gray16_3x5", "one_1x1_rgb", "filters_5rows_rgb"):
        frame, kind, s = ec.cases()[name][0]
        info = ec.encode_info(frame, kind, s)
        data = png_ops.png_file_bytes(info["height"], info["width"], kind, info["zstream"])
        assert data == info["file"]
        assert Image.open(io.BytesIO(data)).size == (info["width"], info["height"])
        assert png_ops.parse_png(data) is not None or kind == ec.GRAY16   # our own reader takes the RGB files
    with pytest.raises(ValueError):
        png_ops.png_file_bytes(1, 1, 7, b"")


def test_options_parse_device_png_encode():
    from monodepth2_amd.options import MonodepthOptions
    opt = MonodepthOptions().parse([])
    assert opt.device_png_encode is False and opt.device_png is False
    opt = MonodepthOptions().parse(["--device_png_encode"])
    assert opt.device_png_encode is True and opt.device_png is False      # the input flag keeps its meaning
    opt = MonodepthOptions().parse(["--device_png"])
    assert opt.device_png is True and opt.device_png_encode is False


def test_default_writers_are_unchanged(tmp_path):
    from PIL import Image
    from monodepth2_amd import eval_ops
    maps = np.arange(2 * 6 * 9, dtype=np.uint16).reshape(2, 6, 9) * 500
    paths = eval_ops.write_benchmark_pngs(maps, str(tmp_path / "a"))
    for p, a in zip(paths, maps):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "PNG")
        assert open(p, "rb").read() == buf.getvalue()
