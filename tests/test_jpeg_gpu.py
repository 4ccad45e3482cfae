"""The JPEG decoder on the device (csrc/jpeg.hip through jpeg_ops.decode_jpeg_batch) against
Pillow: every supported case byte-identical to np.asarray(Image.open(...).convert("RGB")),
alone and in one mixed batch, in any order, twice the same, with nothing written outside
the frames, and a cut stream reported without harm to its neighbours."""
import numpy as np
import pytest
import torch

from monodepth2_amd.build import build
from monodepth2_amd.jpeg_ops import decode_jpeg_batch, parse_jpeg

import jpeg_case as jc

pytestmark = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope="module")
def dev():
    build()
    return torch.device("cuda", torch.cuda.current_device())


def layout(streams, gap=16):
    """16-byte aligned offsets with at least `gap` poison bytes between and after frames."""
    offsets, pos = [], 32
    for s in streams:
        offsets.append(pos)
        pos = (pos + s.height * s.width * 3 + gap + 15) // 16 * 16
    return offsets, pos + 64


def run(streams, dev, check=False, offsets=None):
    if offsets is None:
        offsets, total = layout(streams)
    else:
        total = max(o + s.height * s.width * 3 for o, s in zip(offsets, streams)) + 64
    out = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
    status = decode_jpeg_batch(streams, out, offsets, dev, check=check)
    return out.cpu().numpy(), status.cpu().numpy().copy(), offsets


def frames_and_gaps(out, streams, offsets):
    mask = np.ones(out.size, bool)
    frames = []
    for s, o in zip(streams, offsets):
        n = s.height * s.width * 3
        frames.append(out[o:o + n].reshape(s.height, s.width, 3))
        mask[o:o + n] = False
    return frames, out[mask]


@pytest.mark.parametrize("name", list(jc.cases()))
def test_one_image_per_call_is_byte_identical_to_pillow(dev, name):
    s = jc.parsed(name)
    out, status, offsets = run([s], dev)
    (frame,), rest = frames_and_gaps(out, [s], offsets)
    ref = jc.pillow_rgb(name)
    diff = np.abs(frame.astype(int) - ref)
    print(name, "status", status, "max |diff|", int(diff.max()), "bytes off", int((diff != 0).sum()))
    assert status.tolist() == [0]
    assert np.array_equal(frame, ref)
    assert (rest == POISON).all()


@pytest.fixture(scope="module")
def mixed(dev):
    names = list(jc.cases())
    streams = [jc.parsed(n) for n in names]
    out, status, offsets = run(streams, dev)
    return names, streams, out, status, offsets


def test_all_cases_in_one_batch(mixed):
    names, streams, out, status, offsets = mixed
    frames, rest = frames_and_gaps(out, streams, offsets)
    assert status.tolist() == [0] * len(names)
    bad = [n for n, f in zip(names, frames) if not np.array_equal(f, jc.pillow_rgb(n))]
    assert not bad, bad
    assert (rest == POISON).all()      # between and after the frames: untouched


def test_batch_is_independent_of_order_and_repeatable(dev, mixed):
    names, streams, out, _, offsets = mixed
    again, status, _ = run(streams, dev)
    assert np.array_equal(again, out) and not status.any()          # two runs are bit-equal
    order = np.random.RandomState(3).permutation(len(names)).tolist()
    shuffled = [streams[i] for i in order]
    out2, status2, offsets2 = run(shuffled, dev)
    assert not status2.any()
    frames, _ = frames_and_gaps(out, streams, offsets)
    frames2, rest2 = frames_and_gaps(out2, shuffled, offsets2)
    for k, i in enumerate(order):
        assert np.array_equal(frames2[k], frames[i]), names[i]
    assert (rest2 == POISON).all()


def test_a_cut_stream_is_reported_and_harms_nothing_else(dev):
    good_a, good_b = "size_37x53_422", "noise_64x96_q100_444"
    cut = parse_jpeg(jc.cut_in_half(jc.cases()["size_37x53_420"]))
    assert cut is not None and (cut.height, cut.width) == (37, 53)
    streams = [jc.parsed(good_a), cut, jc.parsed(good_b)]
    out, status, offsets = run(streams, dev)
    frames, rest = frames_and_gaps(out, streams, offsets)
    assert np.array_equal(frames[0], jc.pillow_rgb(good_a))
    assert np.array_equal(frames[2], jc.pillow_rgb(good_b))
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    assert (rest == POISON).all()
    total = max(o + s.height * s.width * 3 for o, s in zip(offsets, streams)) + 64
    buf = torch.zeros(total, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="index 1"):
        decode_jpeg_batch(streams, buf, offsets, dev, check=True)
    good = decode_jpeg_batch([streams[0], streams[2]], buf, [offsets[0], offsets[2]], dev, check=True)
    assert good.tolist() == [0, 0]


def test_arguments_are_checked(dev):
    s = jc.parsed("size_8x8_444")
    out = torch.zeros(1024, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        decode_jpeg_batch([s], out, [8], dev)
    with pytest.raises(RuntimeError, match="past out_bytes"):
        decode_jpeg_batch([s], out, [1024 - 16], dev)
    with pytest.raises(ValueError, match="uint8"):
        decode_jpeg_batch([s], out.float(), [0], dev)
    assert decode_jpeg_batch([], out, [], dev).numel() == 0
