"""CPU-side checks of the PNG decoder's ABI (md2_png_run, csrc/png.hip): struct layout,
exports, every refusal and its message, the workspace query, the GPU-only error of
decode_png_batch and the --device_png flag — no kernel is launched."""
import ctypes

import pytest
import torch

from monodepth2_amd import _lib, build as build_mod
from monodepth2_amd.build import build

NAMES = {"md2_png_workspace_bytes", "md2_png_check", "md2_png_run"}


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def image(height=375, width=1242, stream_bytes=200000, stream_offset=0, out_offset=0):
    im = _lib.PngImage()
    im.height, im.width, im.stream_bytes = height, width, stream_bytes
    im.stream_offset, im.out_offset = stream_offset, out_offset
    return im


def batch(*ims):
    return (_lib.PngImage * len(ims))(*ims)


def check(L, ims, streams_bytes=1 << 20, out_bytes=1 << 23, n=None):
    return L.md2_png_check(ims, len(ims) if n is None else n, streams_bytes, out_bytes)


def test_struct_layout_and_exports(L):
    I = _lib.PngImage
    assert ctypes.sizeof(I) == 32
    assert (I.height.offset, I.width.offset, I.out_offset.offset, I.stream_offset.offset) == (0, 4, 8, 16)
    assert (I.stream_bytes.offset, I.reserved.offset) == (24, 28)
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert NAMES <= set(_lib.EXPORTS)
    for n in NAMES:
        assert hasattr(L, n), n
    assert "png.hip" in build_mod.SOURCES
    assert (_lib.PNG_ST_BLOCK, _lib.PNG_ST_CODE, _lib.PNG_ST_END, _lib.PNG_ST_DIST, _lib.PNG_ST_FILTER,
            _lib.PNG_ST_ADLER) == (1, 2, 4, 8, 16, 32)


def test_a_good_batch_passes(L):
    ims = batch(image(), image(192, 320, 250000, 200000, 375 * 1242 * 3 + 14), image(1, 1, 0, 16 * 30000, 16 * 300000))
    assert check(L, ims) == 0
    assert check(L, batch(image(8192, 8192)), out_bytes=3 * 8192 * 8192) == 0
    assert check(L, ims, n=0) == 0


def refused(L, msg, ims, **kw):
    assert check(L, ims, **kw) == -1
    assert msg in L.md2_last_error().decode()
    # md2_png_run refuses the same batch before it touches a pointer: these addresses must
    # never be dereferenced
    x = ctypes.c_void_p(4096)
    rc = L.md2_png_run(x, kw.get("streams_bytes", 1 << 20), ims, x, kw.get("n", len(ims)), x, 1 << 30, x,
                       kw.get("out_bytes", 1 << 23), x, None)
    assert rc == -1 and msg in L.md2_last_error().decode()


@pytest.mark.parametrize("kw", [dict(height=0), dict(height=8193), dict(width=0), dict(width=-3), dict(width=8193)])
def test_sizes_outside_1_to_8192_are_refused(L, kw):
    refused(L, "1..8192", batch(image(16, 16, 100), image(**kw)))
    assert L.md2_png_workspace_bytes(batch(image(16, 16, 100), image(**kw)), 2) == 0
    assert "1..8192" in L.md2_last_error().decode()


@pytest.mark.parametrize("kw", [dict(stream_offset=8), dict(out_offset=8), dict(out_offset=4097)])
def test_offsets_that_are_no_multiple_of_16_are_refused(L, kw):
    refused(L, "multiples of 16", batch(image(16, 16, 100), image(**kw)))


@pytest.mark.parametrize("kw,ckw", [(dict(stream_offset=(1 << 20) - 992), {}), (dict(stream_offset=1 << 21), {}),
                                    (dict(stream_bytes=1001), dict(streams_bytes=1000))])
def test_streams_outside_streams_bytes_are_refused(L, kw, ckw):
    refused(L, "past streams_bytes", batch(image(16, 16, 100), image(**kw)), **ckw)


@pytest.mark.parametrize("kw,ckw", [(dict(out_offset=(1 << 23) - 1024), {}), (dict(out_offset=1 << 24), {}),
                                    (dict(height=2, width=3), dict(out_bytes=17))])
def test_frames_outside_out_bytes_are_refused(L, kw, ckw):
    refused(L, "past out_bytes", batch(image(1, 1, 100), image(**kw)), **ckw)
    assert check(L, batch(image(2, 3, 10)), out_bytes=18) == 0


def test_a_negative_count_too_many_images_and_null(L):
    ims = batch(image(16, 16, 100))
    for n in (-1, 4097):
        refused(L, "0..4096", ims, n=n)
        assert L.md2_png_workspace_bytes(ims, n) == 0 and "0..4096" in L.md2_last_error().decode()
    assert L.md2_png_check(None, 1, 1, 1) == -1 and "NULL" in L.md2_last_error().decode()
    assert L.md2_png_workspace_bytes(None, 1) == 0
    x = ctypes.c_void_p(4096)
    good = [x, 1 << 20, ims, x, 1, x, 1 << 20, x, 1 << 20, x, None]
    for hole in (0, 3, 5, 7, 9):
        args = list(good)
        args[hole] = None
        assert L.md2_png_run(*args) == -1 and "NULL" in L.md2_last_error().decode()
    args = list(good)
    args[0] = ctypes.c_void_p(4100)
    assert L.md2_png_run(*args) == -1 and "aligned" in L.md2_last_error().decode()
    args = list(good)
    args[6] = 16 * 49 - 1
    assert L.md2_png_run(*args) == -1 and "workspace" in L.md2_last_error().decode()


def test_the_workspace_holds_the_inflated_scanlines(L):
    shapes = [(1, 1), (5, 1), (1, 7), (66, 67), (375, 1242), (8192, 8192)]
    total = 0
    for n, (h, w) in enumerate(shapes, 1):
        ims = batch(*[image(a, b, 10) for a, b in shapes[:n]])
        total += h * (1 + 3 * w)
        need = L.md2_png_workspace_bytes(ims, n)
        assert total <= need <= total + 16 * n and need % 16 == 0
    assert L.md2_png_workspace_bytes(batch(image()), 0) == 0    # nothing to decode, nothing needed


def test_decode_png_batch_is_gpu_only():
    from monodepth2_amd.png_ops import PngStream, decode_png_batch
    s = PngStream(1, 1, b"\x63\x60\x60\x60\x00\x00\x00\x04\x00\x01")
    with pytest.raises(RuntimeError, match="GPU only"):
        decode_png_batch([s], torch.zeros(64, dtype=torch.uint8), [0])
    with pytest.raises(RuntimeError, match="GPU only"):
        decode_png_batch([s], torch.zeros(64, dtype=torch.uint8), [0], device="cpu")


def test_options_parse_device_png():
    from monodepth2_amd.options import MonodepthOptions
    assert MonodepthOptions().parse([]).device_png is False
    assert MonodepthOptions().parse(["--device_png"]).device_png is True
