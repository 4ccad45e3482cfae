"""CPU-side checks of the indexed PNG decoder's ABI (md2_png_index, md2_png_run_indexed,
csrc/png.hip): exports, the index size against the layout, every refusal of
md2_png_check_indexed and of the calls themselves with its message, the workspace query, the
GPU-only errors and pack_dataset's flags — no kernel is launched."""
import ctypes

import numpy as np
import pytest
import torch

from monodepth2_amd import _lib
from monodepth2_amd.build import build

NAMES = {"md2_png_index_bytes", "md2_png_indexed_workspace_bytes", "md2_png_index", "md2_png_check_indexed",
         "md2_png_run_indexed"}


@pytest.fixture(scope="module")
def L():
    build()
    return _lib.lib()


def image(height=24, width=100, stream_bytes=5000, stream_offset=0, out_offset=0):
    im = _lib.PngImage()
    im.height, im.width, im.stream_bytes = height, width, stream_bytes
    im.stream_offset, im.out_offset = stream_offset, out_offset
    return im


def batch(*ims):
    return (_lib.PngImage * len(ims))(*ims)


def offsets(*vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def check(L, ims, offs, segment_bytes=1024, streams_bytes=1 << 20, out_bytes=1 << 23, n=None):
    return L.md2_png_check_indexed(ims, offs, len(ims) if n is None else n, segment_bytes, streams_bytes, out_bytes)


def test_exports_and_constants(L):
    assert L.md2_abi_version() == 24 == _lib.ABI_VERSION   # new symbols only: no bump
    assert NAMES <= set(_lib.EXPORTS)
    for n in NAMES:
        assert hasattr(L, n), n
    assert _lib.PNG_ST_INDEX == 64
    from monodepth2_amd.png_ops import status_text
    assert "index" in status_text(64) and "index" in status_text(64 | 4) and "index" not in status_text(4)


@pytest.mark.parametrize("size", [(1, 1), (24, 100), (375, 1242), (8192, 8192)])
@pytest.mark.parametrize("segment_bytes", [1024, 2048, 4096, 8192, 16384, 32768])
def test_index_bytes_follow_the_layout(L, size, segment_bytes):
    from monodepth2_amd.png_ops import index_nbytes
    h, w = size
    cap = h * (1 + 3 * w) // segment_bytes + 1
    want = (16 + 24 * cap + 15) // 16 * 16
    assert L.md2_png_index_bytes(h, w, segment_bytes) == want == index_nbytes(h, w, segment_bytes)


@pytest.mark.parametrize("bad", [0, 512, 1000, 1025, 3000, 65536, -1024])
def test_a_bad_segment_bytes_is_refused(L, bad):
    ims, offs = batch(image()), offsets(5008)
    msg = "power of two in 1024..32768"
    assert L.md2_png_index_bytes(24, 100, bad) == 0 and msg in L.md2_last_error().decode()
    assert L.md2_png_indexed_workspace_bytes(ims, 1, bad) == 0 and msg in L.md2_last_error().decode()
    assert check(L, ims, offs, segment_bytes=bad) == -1 and msg in L.md2_last_error().decode()
    x = ctypes.c_void_p(4096)
    assert L.md2_png_run_indexed(x, 1 << 20, ims, x, offs, x, 1, bad, x, 1 << 30, x, 1 << 23, x, None) == -1
    assert msg in L.md2_last_error().decode()
    assert L.md2_png_index(x, 1 << 20, ims, x, 1, bad, x, 1 << 20, offs, x, x, None) == -1
    assert msg in L.md2_last_error().decode()


def test_a_good_batch_passes(L):
    nb = L.md2_png_index_bytes(24, 100, 1024)
    ims = batch(image(), image(24, 100, 5000, 16384, 7200 + 16))
    assert check(L, ims, offsets(5008, 16384 + 5008)) == 0
    assert check(L, ims, offsets(5008, (1 << 20) - nb)) == 0       # the last index ends with the buffer
    assert check(L, ims, None, n=0) == 0


def refused(L, msg, ims, offs, **kw):
    assert check(L, ims, offs, **kw) == -1
    assert msg in L.md2_last_error().decode()
    x = ctypes.c_void_p(4096)    # never dereferenced: the call refuses the batch before it touches a pointer
    n = kw.get("n", len(ims))
    rc = L.md2_png_run_indexed(x, kw.get("streams_bytes", 1 << 20), ims, x, offs, x, n, kw.get("segment_bytes", 1024),
                               x, 1 << 30, x, kw.get("out_bytes", 1 << 23), x, None)
    assert rc == -1 and msg in L.md2_last_error().decode()


def test_what_md2_png_check_refuses_is_refused(L):
    offs = offsets(5008, 16384 + 5008)
    refused(L, "1..8192", batch(image(), image(height=0, stream_offset=16384)), offs)
    refused(L, "1..8192", batch(image(), image(width=8193, stream_offset=16384)), offs)
    refused(L, "multiples of 16", batch(image(), image(stream_offset=16392)), offs)
    refused(L, "multiples of 16", batch(image(), image(stream_offset=16384, out_offset=8)), offs)
    refused(L, "past streams_bytes", batch(image(), image(stream_offset=1 << 21)), offs)
    refused(L, "past out_bytes", batch(image(), image(stream_offset=16384, out_offset=1 << 24)), offs)
    refused(L, "0..4096", batch(image()), offsets(5008), n=-1)
    refused(L, "0..4096", batch(image()), offsets(5008), n=4097)
    assert L.md2_png_check_indexed(None, offsets(0), 1, 1024, 1, 1) == -1 and "NULL" in L.md2_last_error().decode()


def test_index_offsets_are_checked(L):
    ims = batch(image(), image(stream_offset=16384, out_offset=7200 + 16))
    nb = L.md2_png_index_bytes(24, 100, 1024)
    assert check(L, ims, None) == -1 and "index_offsets is NULL" in L.md2_last_error().decode()
    refused(L, "index offset must be a multiple of 16", ims, offsets(5008, 16384 + 5000))
    refused(L, "index reaches past streams_bytes", ims, offsets(5008, (1 << 20) - nb + 16))
    refused(L, "index reaches past streams_bytes", ims, offsets(5008, 1 << 21))
    refused(L, "index reaches past streams_bytes", ims, offsets(1 << 40, 16384 + 5008))
    # the same index is longer at a smaller segment_bytes
    assert check(L, ims, offsets(5008, (1 << 20) - nb), segment_bytes=2048) == 0


def test_null_misaligned_and_short_arguments_of_the_calls(L):
    ims, offs = batch(image()), offsets(5008)
    x = ctypes.c_void_p(4096)
    need = L.md2_png_indexed_workspace_bytes(ims, 1, 1024)
    good = [x, 1 << 20, ims, x, offs, x, 1, 1024, x, need, x, 1 << 20, x, None]
    for hole in (0, 3, 4, 5, 8, 10, 12):
        args = list(good)
        args[hole] = None
        assert L.md2_png_run_indexed(*args) == -1 and "NULL" in L.md2_last_error().decode(), hole
    for hole, bad in ((0, 4100), (8, 4104), (3, 4100), (5, 4100)):
        args = list(good)
        args[hole] = ctypes.c_void_p(bad)
        assert L.md2_png_run_indexed(*args) == -1 and "aligned" in L.md2_last_error().decode(), hole
    args = list(good)
    args[9] = need - 1
    assert L.md2_png_run_indexed(*args) == -1 and "workspace" in L.md2_last_error().decode()
    good = [x, 1 << 20, ims, x, 1, 1024, x, 1 << 20, offsets(0), x, x, None]
    for hole in (0, 3, 6, 8, 9, 10):
        args = list(good)
        args[hole] = None
        assert L.md2_png_index(*args) == -1 and "NULL" in L.md2_last_error().decode(), hole
    args = list(good)
    args[7] = L.md2_png_index_bytes(24, 100, 1024) - 1
    assert L.md2_png_index(*args) == -1 and "past index_bytes" in L.md2_last_error().decode()
    args = list(good)
    args[8] = offsets(8)
    assert L.md2_png_index(*args) == -1 and "multiple of 16" in L.md2_last_error().decode()
    assert L.md2_png_run_indexed(x, 1, ims, x, offs, x, 0, 1024, x, 0, x, 0, x, None) == 0   # nothing to do


def test_the_workspace_holds_scanlines_symbols_and_segment_words(L):
    shapes = [(1, 1), (24, 100), (66, 67), (375, 1242)]
    for s in (1024, 16384):
        ims = batch(*[image(h, w, 10) for h, w in shapes])
        scan = L.md2_png_workspace_bytes(ims, len(shapes))
        words = sum(h * (1 + 3 * w) // s + 1 for h, w in shapes)
        assert L.md2_png_indexed_workspace_bytes(ims, len(shapes), s) == 3 * scan + (4 * words + 15) // 16 * 16
    assert L.md2_png_indexed_workspace_bytes(batch(image(0, 1)), 1, 1024) == 0
    assert "1..8192" in L.md2_last_error().decode()


def test_the_indexed_entry_points_are_gpu_only():
    from monodepth2_amd.png_ops import PngStream, decode_png_batch_indexed, index_nbytes
    s = PngStream(1, 1, b"\x63\x60\x60\x60\x00\x00\x00\x04\x00\x01")
    ix = np.zeros(index_nbytes(1, 1, 1024), np.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        decode_png_batch_indexed([s], [ix], torch.zeros(64, dtype=torch.uint8), [0])
    with pytest.raises(RuntimeError, match="GPU only"):
        decode_png_batch_indexed([s], [ix], torch.zeros(64, dtype=torch.uint8), [0], device="cpu")
    from monodepth2_amd.png_ops import index_png_batch
    with pytest.raises(RuntimeError, match="GPU only"):
        index_png_batch([s], 1024, device="cpu")


def test_png_records_and_transcode_exclude_each_other(tmp_path, capsys):
    from monodepth2_amd.pack import build_pack
    from monodepth2_amd.pack_dataset import main
    with pytest.raises(ValueError, match="png_records and transcode"):
        build_pack(str(tmp_path / "x.pack"), str(tmp_path), [[]], png=True, png_records=True, transcode=(92, "420"))
    with pytest.raises(SystemExit):
        main(["--data_path", str(tmp_path), "--lists", "none.txt", "--out", str(tmp_path / "x.pack"), "--png",
              "--png_records", "--transcode"])
    assert "--png_records and --transcode" in capsys.readouterr().err
    with pytest.raises(ValueError, match="power of two"):
        build_pack(str(tmp_path / "x.pack"), str(tmp_path), [[]], png=True, png_records=True, segment_bytes=1000)
