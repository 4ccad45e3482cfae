"""CPU-side checks of the indexed JPEG decoder's ABI (md2_jpeg_index, md2_jpeg_run_indexed,
csrc/jpeg.hip), in the manner of test_jpeg_abi.py: exports, the index size, every refusal
and its message — no kernel is launched and no plan is created."""
import ctypes

import pytest
import torch  # noqa: F401  (load order: torch's HIP runtime first)

from monodepth2_amd import _lib, jpeg_ops
from monodepth2_amd.build import build

from test_jpeg_abi import batch, image

NAMES = {"md2_jpeg_index_bytes", "md2_jpeg_index", "md2_jpeg_check_indexed", "md2_jpeg_run_indexed"}


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def u64(*values):
    return (ctypes.c_uint64 * len(values))(*values)


def test_exports_and_abi(L):
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert NAMES <= set(_lib.EXPORTS)
    for n in NAMES:
        assert hasattr(L, n), n
    assert ctypes.sizeof(_lib.JpegImage) == 48              # the index offsets travel beside it
    assert _lib.JPEG_ST_INDEX == 8 and not _lib.JPEG_ST_INDEX & (_lib.JPEG_ST_BLOCKS | _lib.JPEG_ST_CODE |
                                                                  _lib.JPEG_ST_END)


def test_index_bytes_is_twelve_per_subsequence_padded_to_sixteen(L):
    for nbytes in (0, 1, 127, 128, 129, 256, 257, 384, 385, 512, 513, 200000, 1 << 28):
        nsub = max(-(-8 * nbytes // 1024), 1)
        assert L.md2_jpeg_index_bytes(nbytes) == (12 * nsub + 15) // 16 * 16 == jpeg_ops.index_nbytes(nbytes), nbytes
        assert jpeg_ops.index_nsub(nbytes) == nsub


def good():
    """Two images whose streams and indexes share one buffer of 1 << 20 bytes: stream, index, stream, index."""
    a, b = image(16, 16, _lib.JPEG_420, 100), image(375, 1242, _lib.JPEG_422, 200000, 256, 16 * 1024)
    return batch(a, b), u64(112, 256 + 200000), (16, (200000 * 8 + 1023) // 1024 * 12 + 15 & ~15)


def check(L, ims, ix, num_quant=2, num_huff=4, streams_bytes=1 << 20, out_bytes=1 << 23):
    return L.md2_jpeg_check_indexed(ims, ix, len(ims), num_quant, num_huff, streams_bytes, out_bytes)


def run(L, ims, ix, streams_bytes=1 << 20, out_bytes=1 << 23, n=None, streams=4096):
    """md2_jpeg_run_indexed on addresses that must never be dereferenced."""
    x = ctypes.c_void_p(4096)
    bank = _lib.JpegBank(4096, 8192, 2, 4)
    return L.md2_jpeg_run_indexed(x, ctypes.c_void_p(streams), streams_bytes, ims, ix, len(ims) if n is None else n,
                                  ctypes.byref(bank), x, out_bytes, x, None)


def test_a_good_batch_passes_and_the_last_byte_counts(L):
    ims, ix, sizes = good()
    assert check(L, ims, ix) == 0
    end = 256 + 200000 + sizes[1]
    assert check(L, ims, ix, streams_bytes=end) == 0
    assert check(L, ims, ix, streams_bytes=end - 1) == -1 and "index reaches past streams_bytes" in L.md2_last_error().decode()
    # an empty stream still has one subsequence: 16 bytes of index
    one = batch(image(1, 1, _lib.JPEG_420, 0))
    assert check(L, one, u64(0), streams_bytes=16) == 0
    assert check(L, one, u64(0), streams_bytes=15) == -1 and "index reaches past" in L.md2_last_error().decode()


BAD = [
    (lambda ims, ix: ix.__setitem__(1, 256 + 200000 + 8), {}, "index offset must be a multiple of 16"),
    (lambda ims, ix: ix.__setitem__(0, 100), {}, "index offset must be a multiple of 16"),
    (lambda ims, ix: ix.__setitem__(1, (1 << 20) - 16), {}, "index reaches past streams_bytes"),
    (lambda ims, ix: ix.__setitem__(0, 1 << 20), {}, "index reaches past streams_bytes"),
    (lambda ims, ix: ix.__setitem__(0, 1 << 40), {}, "index reaches past streams_bytes"),
    (lambda ims, ix: None, dict(streams_bytes=256 + 200000 + 32), "index reaches past streams_bytes"),
    # what md2_jpeg_run refuses is refused here too, first
    (lambda ims, ix: setattr(ims[1], "stream_offset", 6), {}, "multiple of 4"),
    (lambda ims, ix: setattr(ims[1], "out_offset", 8), {}, "multiple of 16"),
    (lambda ims, ix: setattr(ims[1], "height", 0), {}, "1..8192"),
    (lambda ims, ix: setattr(ims[1], "sampling", 3), {}, "sampling"),
    (lambda ims, ix: setattr(ims[1], "stream_offset", (1 << 20) - 1000), {}, "past streams_bytes"),
    (lambda ims, ix: None, dict(out_bytes=1 << 20), "past out_bytes"),
]


@pytest.mark.parametrize("spoil,ckw,msg", BAD)
def test_refusals_name_their_reason_and_launch_nothing(L, spoil, ckw, msg):
    ims, ix, _ = good()
    spoil(ims, ix)
    assert check(L, ims, ix, **ckw) == -1
    assert msg in L.md2_last_error().decode()
    # md2_jpeg_run_indexed refuses the same batch before it looks at its plan
    assert run(L, ims, ix, **ckw) == -1 and msg in L.md2_last_error().decode()
    # and so does md2_jpeg_index, whose indexes lie in a buffer of their own (it writes no frame)
    if "index" in msg:
        x = ctypes.c_void_p(4096)
        bank = _lib.JpegBank(4096, 8192, 2, 4)
        rc = L.md2_jpeg_index(x, x, 1 << 20, ims, ix, 2, ctypes.byref(bank), x, ckw.get("streams_bytes", 1 << 20), x, None)
        assert rc == -1 and msg.replace("streams_bytes", "index_bytes") in L.md2_last_error().decode()


def test_null_arrays_counts_and_alignment(L):
    ims, ix, _ = good()
    assert L.md2_jpeg_check_indexed(None, ix, 2, 2, 4, 1 << 20, 1 << 23) == -1 and "NULL" in L.md2_last_error().decode()
    assert L.md2_jpeg_check_indexed(ims, None, 2, 2, 4, 1 << 20, 1 << 23) == -1
    assert "index_offsets" in L.md2_last_error().decode() and "NULL" in L.md2_last_error().decode()
    x = ctypes.c_void_p(4096)
    bank = _lib.JpegBank(4096, 8192, 2, 4)
    good_run = [x, x, 1 << 20, ims, ix, 2, ctypes.byref(bank), x, 1 << 23, x, None]
    good_index = [x, x, 1 << 20, ims, ix, 2, ctypes.byref(bank), x, 1 << 20, x, None]
    for fn, args in ((L.md2_jpeg_run_indexed, good_run), (L.md2_jpeg_index, good_index)):
        for hole in (0, 1, 3, 4, 6, 7, 9):
            a = list(args)
            a[hole] = None
            assert fn(*a) == -1 and "NULL" in L.md2_last_error().decode(), hole
        for q, h in ((None, 8192), (4096, None)):
            b = _lib.JpegBank(q, h, 2, 4)
            a = list(args)
            a[6] = ctypes.byref(b)
            assert fn(*a) == -1 and "bank." in L.md2_last_error().decode()
        for n, msg in ((0, "at least one"), (-1, "at least one"), (4097, "too many")):
            a = list(args)
            a[5] = n
            assert fn(*a) == -1 and msg in L.md2_last_error().decode()
    for n, msg in ((0, "at least one"), (4097, "too many")):
        assert L.md2_jpeg_check_indexed(ims, ix, n, 2, 4, 1 << 20, 1 << 23) == -1 and msg in L.md2_last_error().decode()
    # the states are 64-bit words read in place: a streams pointer that would misalign them
    assert run(L, ims, ix, streams=4096 + 8) == -1 and "16-byte aligned" in L.md2_last_error().decode()
    a = list(good_index)
    a[7] = ctypes.c_void_p(4096 + 8)
    assert L.md2_jpeg_index(*a) == -1 and "16-byte aligned" in L.md2_last_error().decode()


def test_describe_batch_indexed_puts_every_index_behind_its_stream():
    import jpeg_case as jc
    names = ["flat_16x16_420", "size_1x1_444", "mix_24x40_422_q100", "noise_64x96_q100_444"]
    streams = [jc.parsed(n) for n in names]
    images, ix, quant, huff, base, total = jpeg_ops.describe_batch_indexed(streams, [0, 256, 512, 4096])
    pos = 0
    for i, s in enumerate(streams):
        assert images[i].stream_offset == pos and images[i].stream_bytes == len(s.data)
        pos += (len(s.data) + 15) // 16 * 16
        assert ix[i] == pos
        pos += jpeg_ops.index_nbytes(len(s.data))
    assert total == base + pos and base % 16 == 0
    jpeg_ops.check_described_indexed(images, ix, len(streams), len(quant), len(huff), total - base, 1 << 16)
    with pytest.raises(RuntimeError, match="index reaches past"):
        jpeg_ops.check_described_indexed(images, ix, len(streams), len(quant), len(huff), total - base - 16, 1 << 16)
