"""loader.BatchLoader(device_png=True), convert_files(device_png=True) and build_pack(...,
device_png=True) against their PIL routes on a synthetic KITTI tree of PNGs (tests/
kitti_tree.py): every tensor of every batch bit-equal with no frame left to PIL; gray and
interlaced files inside a device-decoded batch go through PIL and change nothing; a damaged
stream is reported by name; the converted .jpg files and the transcoded pack are the same
bytes with the flag as without."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import kitti_tree as KT
import png_case as pc

from test_loader_jpeg_gpu import FRAME_IDS, assert_same, dataset

pytestmark = pytest.mark.gpu


def pngs_of(root):
    return sorted(os.path.join(d, f) for d, _, files in os.walk(root) for f in files if f.endswith(".png"))


def batches(ds, threads, device_png, **kw):
    """(batches, frames PIL decoded) of one epoch."""
    from monodepth2_amd.loader import BatchLoader
    ld = BatchLoader(ds, 2, shuffle=False, seed=5, num_workers=threads, device_png=device_png, **kw)
    try:
        out = list(ld)
        torch.cuda.synchronize()
    finally:
        ld.close()
    return out, ld.pil_fallbacks


@pytest.fixture(scope="module")
def png_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_png"))
    KT.write_tree(root, ext=".png")
    return root


@pytest.fixture(scope="module")
def pil_batches(png_tree):
    """the flag-off batches, computed once and never changed"""
    return batches(dataset(png_tree, ext=".png"), 0, False)[0]


@pytest.mark.parametrize("threads", [0, 4])
def test_device_decoded_png_batches_are_bit_equal_to_pil(png_tree, pil_batches, threads):
    got, fallbacks = batches(dataset(png_tree, ext=".png"), threads, True)
    assert fallbacks == 0
    assert_same(got, pil_batches)


def test_the_tail_batch_and_the_flag_implies_device_decode(png_tree):
    from monodepth2_amd.loader import BatchLoader
    got, fallbacks = batches(dataset(png_tree, ext=".png"), 2, True, drop_last=False)
    want, _ = batches(dataset(png_tree, ext=".png"), 2, False, drop_last=False)
    assert len(got) == 3 and fallbacks == 0
    assert_same(got, want)
    ld = BatchLoader(dataset(png_tree, ext=".png"), 2, device_png=True)
    assert ld.device_decode and ld.device_png
    ld.close()


def test_gray_and_interlaced_files_go_through_pil(tmp_path):
    from monodepth2_amd.png_ops import parse_png
    root = str(tmp_path)
    KT.write_tree(root, ext=".png")
    folder = os.path.join(root, KT.DRIVES[1][0], "image_02/data")
    gray = os.path.join(folder, "%010d.png" % 0)
    Image.open(gray).convert("L").save(gray)
    laced = os.path.join(folder, "%010d.png" % 2)
    img = np.asarray(Image.open(laced).convert("RGB"))
    h, w = img.shape[:2]       # Pillow reads interlaced files and does not write them: written here
    with open(laced, "wb") as f:
        f.write(interlaced_png(img))
    assert parse_png(open(gray, "rb").read()) is None and parse_png(open(laced, "rb").read()) is None
    assert np.array_equal(np.asarray(Image.open(laced).convert("RGB")), img) and (h, w) == KT.DRIVES[1][1]
    got, fallbacks = batches(dataset(root, ext=".png"), 2, True)
    want, none = batches(dataset(root, ext=".png"), 2, False)
    # the split lines name drive 1's left camera once: frames 0, 1, 2 of it are one item
    assert fallbacks == 2 and none == 0
    assert_same(got, want)


def interlaced_png(img):
    """An Adam7-interlaced 8-bit RGB file of `img` (filter None on every row of every pass)."""
    h, w, _ = img.shape
    passes = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]
    raw = bytearray()
    for x0, y0, dx, dy in passes:
        sub = img[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            for row in sub:
                raw.append(0)
                raw += row.tobytes()
    return b"".join([pc.SIGNATURE, pc.ihdr(h, w, interlace=1), pc.chunk(b"IDAT", pc.zlib_stream(bytes(raw))),
                     pc.chunk(b"IEND")])


def test_a_damaged_stream_is_reported_by_name(tmp_path):
    root = str(tmp_path)
    KT.write_tree(root, ext=".png")
    bad = os.path.join(root, KT.DRIVES[1][0], "image_02/data", "%010d.png" % 2)
    img = np.asarray(Image.open(bad).convert("RGB"))
    h, w = img.shape[:2]
    raw = pc.filter_rows(img, [pc.SUB] * h)
    with open(bad, "wb") as f:
        f.write(pc.png_bytes(h, w, pc.zlib_stream(raw[:(h - 1) * (1 + 3 * w)])))      # a row short: ST_END
    for threads in (0, 2):
        with pytest.raises(RuntimeError, match="did not decode") as e:
            batches(dataset(root, ext=".png"), threads, True)
        text = str(e.value)
        assert "%010d.png" % 2 in text and KT.DRIVES[1][0] in text and "split line 1" in text and "status 4" in text


def test_convert_files_writes_the_same_bytes(tmp_path):
    from monodepth2_amd.convert_dataset import convert_files, main
    roots = []
    for name in ("off", "on"):
        root = str(tmp_path / name)
        KT.write_tree(root, ext=".png")
        gray = os.path.join(root, KT.DRIVES[0][0], "image_03/data", "%010d.png" % 1)
        Image.open(gray).convert("L").save(gray)                          # one file for PIL on either route
        roots.append(root)
    off = convert_files(pngs_of(roots[0]), batch=5, threads=3)
    on = convert_files(pngs_of(roots[1]), batch=5, threads=3, device_png=True)
    assert on["device_decoded"] == 11 and "device_decoded" not in off
    assert {k: on[k] for k in off} == off and off["converted"] == 12
    for a, b in zip(pngs_of(roots[0]), pngs_of(roots[1])):
        with open(a[:-4] + ".jpg", "rb") as fa, open(b[:-4] + ".jpg", "rb") as fb:
            assert fa.read() == fb.read(), a
    stats = main(["--data_path", roots[1], "--device_png", "--overwrite", "--quality", "75"])
    assert stats["converted"] == 12 and stats["device_decoded"] == 11


def test_a_transcoded_pack_is_the_same_record_for_record(png_tree, tmp_path):
    from monodepth2_amd.pack import FramePack, build_pack
    packs = []
    for name, flag in (("off", False), ("on", True)):
        path = str(tmp_path / (name + ".pack"))
        stats = build_pack(path, png_tree, [KT.LINES], png=True, frame_ids=FRAME_IDS, batch=5, threads=2,
                           transcode=(92, "4:2:0"), device_png=flag)
        assert stats["frames"] == stats["jpeg"] == stats["transcoded"] == 12
        packs.append((FramePack(path), stats))
    (a, sa), (b, sb) = packs
    assert sa == sb and list(a.names) == list(b.names)
    assert a.records.tobytes() == b.records.tobytes()
    for key in a.names:
        (s, i), (t, j) = a.stream(key), b.stream(key)
        assert s.data == t.data and s.quant == t.quant and np.array_equal(i, j)
    with open(str(tmp_path / "off.pack"), "rb") as fa, open(str(tmp_path / "on.pack"), "rb") as fb:
        assert fa.read() == fb.read()
