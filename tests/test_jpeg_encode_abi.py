"""CPU-side checks of the JPEG encoder's ABI (md2_jpeg_encode, csrc/jpegenc.hip), in the
manner of test_jpeg_abi.py: exports, the capacity bound, the workspace size and every
refusal with its message — no kernel is launched."""
import ctypes

import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib, jpeg_ops
from monodepth2_amd.build import build

NAMES = {"md2_jpeg_encode_bound", "md2_jpeg_encode_workspace_bytes", "md2_jpeg_encode_check", "md2_jpeg_encode"}


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def image(h, w, sampling, in_offset=0, out_offset=0, cap=None, quant=(0, 1)):
    im = _lib.JpegEncImage()
    im.height, im.width, im.sampling = h, w, sampling
    im.in_offset, im.out_offset = in_offset, out_offset
    im.out_capacity = blocks(h, w, sampling) * 208 if cap is None else cap
    im.quant[0], im.quant[1] = quant
    return im


def batch(*ims):
    return (_lib.JpegEncImage * len(ims))(*ims)


def blocks(h, w, sampling):
    hs, vs = {_lib.JPEG_444: (1, 1), _lib.JPEG_422: (2, 1), _lib.JPEG_420: (2, 2)}[sampling]
    return -(-w // (8 * hs)) * -(-h // (8 * vs)) * (hs * vs + 2)


def check(L, ims, num_quant=2, in_bytes=1 << 24, out_bytes=1 << 24):
    return L.md2_jpeg_encode_check(ims, len(ims), num_quant, in_bytes, out_bytes)


def refused(L, rc, text):
    assert rc == -1
    assert text in L.md2_last_error().decode(), L.md2_last_error().decode()


def test_exports_and_abi(L):
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert NAMES <= set(_lib.EXPORTS)
    for n in NAMES:
        assert hasattr(L, n), n
    assert ctypes.sizeof(_lib.JpegEncImage) == 40
    assert _lib.JPEGENC_ST_SPACE == 1


@pytest.mark.parametrize("h,w", [(1, 1), (8, 8), (9, 3), (16, 16), (17, 33), (24, 40), (375, 1242), (8192, 8192)])
@pytest.mark.parametrize("sampling", [_lib.JPEG_444, _lib.JPEG_422, _lib.JPEG_420])
def test_bound_is_208_bytes_per_block_of_the_scan(L, h, w, sampling):
    """dummy blocks of partial MCUs are coded too, so they count"""
    assert L.md2_jpeg_encode_bound(h, w, sampling) == 208 * blocks(h, w, sampling) == jpeg_ops.encode_bound(h, w, sampling)
    assert 8 * 208 >= 20 + 63 * 26


@pytest.mark.parametrize("h,w,sampling", [(0, 8, 0), (8, 0, 0), (8193, 8, 2), (8, 8193, 1), (8, 8, 3), (8, 8, -1)])
def test_bound_and_workspace_refuse_a_bad_geometry(L, h, w, sampling):
    assert L.md2_jpeg_encode_bound(h, w, sampling) == 0
    assert "jpeg encode" in L.md2_last_error().decode()
    assert L.md2_jpeg_encode_workspace_bytes(batch(image(8, 8, 0), _bad(h, w, sampling)), 2) == 0
    refused(L, check(L, batch(_bad(h, w, sampling))), "1..8192" if sampling in (0, 1, 2) else "sampling")


def _bad(h, w, sampling):
    im = _lib.JpegEncImage()
    im.height, im.width, im.sampling, im.out_capacity = h, w, sampling, 208
    return im


def test_workspace_holds_the_table_coefficients_counts_and_offsets(L):
    ims = batch(image(375, 1242, _lib.JPEG_420), image(17, 33, _lib.JPEG_444))
    need = L.md2_jpeg_encode_workspace_bytes(ims, 2)
    tb = [blocks(375, 1242, _lib.JPEG_420), blocks(17, 33, _lib.JPEG_444)]
    assert need % 256 == 0
    assert need >= sum(t * (128 + 4 + 8) for t in tb)
    assert need <= sum(t * (128 + 4 + 8) for t in tb) + 256 * 8
    assert L.md2_jpeg_encode_workspace_bytes(ims, 0) == 0 and "1..4096" in L.md2_last_error().decode()
    assert L.md2_jpeg_encode_workspace_bytes(None, 1) == 0 and "NULL" in L.md2_last_error().decode()


def test_a_good_batch_passes_and_the_last_byte_counts(L):
    a = image(16, 16, _lib.JPEG_420, 0, 0, cap=100)
    b = image(37, 53, _lib.JPEG_422, 768, 112, cap=1000)
    ims = batch(a, b)
    in_end, out_end = 768 + 37 * 53 * 3, 112 + 1000
    assert check(L, ims, in_bytes=in_end, out_bytes=out_end) == 0
    refused(L, check(L, ims, in_bytes=in_end - 1, out_bytes=out_end), "frame reaches past in_bytes")
    refused(L, check(L, ims, in_bytes=in_end, out_bytes=out_end - 1), "output range reaches past out_bytes")
    refused(L, check(L, batch(image(8, 8, 0, in_offset=1 << 40))), "frame reaches past in_bytes")
    refused(L, check(L, batch(image(8, 8, 0, out_offset=1 << 40))), "output range reaches past out_bytes")


def test_a_range_is_rounded_up_to_whole_words(L):
    """whole 32-bit words take the atomic OR: a capacity of 99 bytes needs 100 of out, rounded
    up likewise"""
    assert check(L, batch(image(16, 16, 2, cap=99)), out_bytes=99) == 0
    assert check(L, batch(image(16, 16, 2, cap=99)), out_bytes=100) == 0
    refused(L, check(L, batch(image(16, 16, 2, cap=99)), out_bytes=98), "output range reaches past out_bytes")
    assert check(L, batch(image(16, 16, 2, cap=0)), out_bytes=0) == 0   # nothing fits: ST_SPACE at run time


@pytest.mark.parametrize("offset", [1, 4, 8, 17])
def test_out_offset_must_be_a_multiple_of_16(L, offset):
    refused(L, check(L, batch(image(8, 8, 0, out_offset=offset))), "multiple of 16")
    assert check(L, batch(image(8, 8, 0, in_offset=offset))) == 0   # frames are tight: any byte offset


def test_table_ids_and_bank_size(L):
    refused(L, check(L, batch(image(8, 8, 0, quant=(0, 2)))), "table index is outside the bank")
    refused(L, check(L, batch(image(8, 8, 0, quant=(2, 0)))), "table index is outside the bank")
    assert check(L, batch(image(8, 8, 0, quant=(0, 2))), num_quant=3) == 0
    refused(L, check(L, batch(image(8, 8, 0)), num_quant=0), "num_quant")
    refused(L, check(L, batch(image(8, 8, 0)), num_quant=257), "num_quant")
    refused(L, L.md2_jpeg_encode_check(None, 1, 2, 1 << 20, 1 << 20), "NULL")
    refused(L, L.md2_jpeg_encode_check(batch(image(8, 8, 0)), 4097, 2, 1 << 20, 1 << 20), "1..4096")


def run(L, ims, workspace_bytes=1 << 30, **kw):
    """md2_jpeg_encode on addresses that must never be dereferenced."""
    args = dict(inp=4096, dev=4096, quant=4096, out=4096, ws=4096, sb=4096, st=4096)
    args.update(kw)
    return L.md2_jpeg_encode(args["inp"], 1 << 24, ims, args["dev"], len(ims), args["quant"], 2, args["out"], 1 << 24,
                             args["ws"], workspace_bytes, args["sb"], args["st"], None)


def test_encode_refuses_before_it_launches(L):
    ims = batch(image(16, 16, 2), image(8, 8, 0, 768, 2048))
    for name in ("inp", "dev", "quant", "out", "ws", "sb", "st"):
        refused(L, run(L, ims, **{name: None}), "NULL")
    refused(L, run(L, ims, out=4100), "aligned")
    refused(L, run(L, ims, ws=4096 + 128), "aligned")
    refused(L, run(L, ims, workspace_bytes=L.md2_jpeg_encode_workspace_bytes(ims, 2) - 1), "more workspace")
    refused(L, run(L, batch(image(16, 16, 2, out_offset=8))), "multiple of 16")
    refused(L, run(L, batch(_bad(16, 16, 5))), "sampling")


def test_wrapper_is_gpu_only():
    with pytest.raises(RuntimeError, match="GPU only"):
        jpeg_ops.encode_jpeg_batch([], device="cpu")
