"""The stored synchronisation index on the device (md2_jpeg_index, md2_jpeg_run_indexed,
csrc/jpeg.hip) on every case of tests/jpeg_case.py, all in ONE batch so that workgroups of
one-subsequence images and of images that span many workgroups interleave:

* index_jpeg_batch equals the host restatement (tests/jpeg_index_case.py) state for state
  and count for count;
* decode_jpeg_batch_indexed gives, frame for frame, Pillow's bytes and decode_jpeg_batch's,
  status 0 everywhere, no byte of `out` outside the frames written, two runs bit-equal;
* a batch with two frames' indexes swapped and one with a frame's index zeroed report
  JPEG_ST_INDEX for those frames and leave every other frame Pillow's.

The cases cover: a stream shorter than one subsequence (flat_16x16_420), the 1x1 images,
partial MCUs in all three samplings, per-file tables (_opt), more subsequences than a
workgroup has threads (noise_192x320_q100_444: 1961, kitti_375x1242_q92_422: 1772)."""
import numpy as np
import pytest
import torch

import jpeg_case as jc
import jpeg_index_case as ic

from monodepth2_amd import _lib, jpeg_ops

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def names():
    got = list(jc.cases())
    for must in ("flat_16x16_420", "size_1x1_444", "size_1x1_422", "size_1x1_420", "size_17x33_444", "size_17x33_422",
                 "size_17x33_420", "mix_24x40_422_q92_opt", "noise_192x320_q100_444", "kitti_375x1242_q92_422"):
        assert must in got
    return got


@pytest.fixture(scope="module")
def streams(names):
    return [jc.parsed(n) for n in names]


@pytest.fixture(scope="module")
def layout(streams):
    """Frame offsets with a gap of 256 untouched bytes between frames, and the buffer's size."""
    offsets, pos = [], 256
    for s in streams:
        offsets.append(pos)
        pos += (s.height * s.width * 3 + 255) // 256 * 256 + 256
    return offsets, pos


@pytest.fixture(scope="module")
def device_indexes(streams):
    return jpeg_ops.index_jpeg_batch(streams, "cuda", check=True)


def decode(fn, streams, layout, *extra):
    offsets, total = layout
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    status = fn(streams, *extra, out, offsets).cpu().numpy().copy()
    return out.cpu().numpy(), status


def frame(buf, layout, streams, i):
    s = streams[i]
    n = s.height * s.width * 3
    return buf[layout[0][i]:layout[0][i] + n].reshape(s.height, s.width, 3)


def outside(buf, layout, streams):
    mask = np.ones(buf.size, bool)
    for o, s in zip(layout[0], streams):
        mask[o:o + s.height * s.width * 3] = False
    return buf[mask]


def test_the_device_index_is_the_restatement(names, streams, device_indexes):
    assert len(device_indexes) == len(names)
    many = 0
    for name, s, idx in zip(names, streams, device_indexes):
        assert idx.dtype == np.uint8 and idx.size == jpeg_ops.index_nbytes(len(s.data)), name
        states, first = jpeg_ops.unpack_index(idx, len(s.data))
        want_states, want_first = ic.restated(name)
        assert states.tolist() == want_states, name
        assert first.tolist() == want_first, name
        assert np.array_equal(idx, ic.restated_bytes(name)), name     # the padding too
        many += len(want_states) > 1024
    assert many >= 2
    assert len(ic.restated("flat_16x16_420")[0]) == 1 and len(jc.parsed("flat_16x16_420").data) < 128


def test_indexing_twice_is_bit_equal_and_a_short_stream_is_reported(streams, device_indexes):
    again = jpeg_ops.index_jpeg_batch(streams, "cuda")
    assert all(np.array_equal(a, b) for a, b in zip(again, device_indexes))
    cut = jpeg_ops.parse_jpeg(jc.cut_in_half(jc.cases()["size_37x53_420"]))
    assert len(jpeg_ops.index_jpeg_batch([cut], "cuda")[0]) == jpeg_ops.index_nbytes(len(cut.data))
    with pytest.raises(RuntimeError, match="does not hold"):
        jpeg_ops.index_jpeg_batch([streams[0], cut], "cuda", check=True)
    assert jpeg_ops.index_jpeg_batch([], "cuda") == []
    # decoded from its own (true) index the short stream is reported as it is without one
    out = torch.zeros(1 << 14, dtype=torch.uint8, device="cuda")
    status = jpeg_ops.decode_jpeg_batch_indexed([streams[0], cut], [device_indexes[0]] + jpeg_ops.index_jpeg_batch(
        [cut], "cuda"), out, [0, 4096]).cpu().tolist()
    plain = jpeg_ops.decode_jpeg_batch([streams[0], cut], out, [0, 4096]).cpu().tolist()
    assert status[0] == plain[0] == 0 and plain[1] & _lib.JPEG_ST_BLOCKS and status[1] & _lib.JPEG_ST_BLOCKS
    with pytest.raises(RuntimeError, match="stream index 1 did not decode"):
        jpeg_ops.decode_jpeg_batch_indexed([streams[0], cut], [device_indexes[0]] + jpeg_ops.index_jpeg_batch(
            [cut], "cuda"), out, [0, 4096], check=True)


@pytest.fixture(scope="module")
def indexed(streams, layout, device_indexes):
    return decode(jpeg_ops.decode_jpeg_batch_indexed, streams, layout, device_indexes)


def test_indexed_decode_is_pillow_and_the_unindexed_decoder_byte_for_byte(names, streams, layout, indexed):
    buf, status = indexed
    ref, ref_status = decode(jpeg_ops.decode_jpeg_batch, streams, layout)
    assert status.tolist() == [0] * len(names) and ref_status.tolist() == [0] * len(names)
    for i, name in enumerate(names):
        assert np.array_equal(frame(buf, layout, streams, i), jc.pillow_rgb(name)), name
    assert np.array_equal(buf, ref)
    assert (outside(buf, layout, streams) == FILL).all()


def test_two_runs_are_bit_equal_and_the_restated_index_decodes_too(names, streams, layout, indexed):
    again, status = decode(jpeg_ops.decode_jpeg_batch_indexed, streams, layout, [ic.restated_bytes(n) for n in names])
    assert status.tolist() == [0] * len(names)
    assert np.array_equal(again, indexed[0])


def spoiled(names, streams, layout, indexes, bad):
    """Decodes with `indexes`; the frames in `bad` must report JPEG_ST_INDEX, all others be Pillow's."""
    buf, status = decode(jpeg_ops.decode_jpeg_batch_indexed, streams, layout, indexes)
    for i, name in enumerate(names):
        if i in bad:
            assert status[i] & _lib.JPEG_ST_INDEX, (name, status[i])
        else:
            assert status[i] == 0, (name, status[i])
            assert np.array_equal(frame(buf, layout, streams, i), jc.pillow_rgb(name)), name
    assert (outside(buf, layout, streams) == FILL).all()


def test_swapped_indexes_are_reported_and_harm_no_other_frame(names, streams, layout, device_indexes):
    # pairs of equal subsequence count (an index has its stream's size): 9 and 6 subsequences
    pairs = [("size_37x53_422", "mix_24x40_420_q100"), ("mix_24x40_444_q92", "mix_24x40_444_q92_opt")]
    indexes, bad = list(device_indexes), set()
    for a, b in pairs:
        i, j = names.index(a), names.index(b)
        assert indexes[i].size == indexes[j].size > 16 and not np.array_equal(indexes[i], indexes[j])
        indexes[i], indexes[j] = indexes[j], indexes[i]
        bad |= {i, j}
    spoiled(names, streams, layout, indexes, bad)


def test_zeroed_and_garbage_indexes_are_reported_and_harm_no_other_frame(names, streams, layout, device_indexes):
    indexes, bad = list(device_indexes), set()
    for name in ("kitti_375x1242_q92_422", "noise_64x96_q100_444", "size_16x16_444"):   # 1772, 197 and 2 subsequences
        i = names.index(name)
        indexes[i] = np.zeros_like(indexes[i])
        bad.add(i)
    # every bit set: states far past the stream, block counts far past the image
    i = names.index("noise_192x320_q100_444")
    indexes[i] = np.full_like(indexes[i], 0xFF)
    bad.add(i)
    # one first_block count off by one in the middle of an otherwise true index
    i = names.index("size_37x53_444")
    n = jpeg_ops.index_nsub(len(streams[i].data))
    states, first = jpeg_ops.unpack_index(indexes[i], len(streams[i].data))
    first[n // 2] += 1
    indexes[i] = jpeg_ops.pack_index(states, first)
    bad.add(i)
    spoiled(names, streams, layout, indexes, bad)
    # a zeroed index of a one-subsequence stream is its true index
    i = names.index("flat_16x16_420")
    assert not device_indexes[i].any()


def test_an_index_of_the_wrong_size_is_refused_on_the_host(streams, layout, device_indexes):
    indexes = list(device_indexes)
    indexes[3] = np.zeros(indexes[3].size + 16, np.uint8)
    with pytest.raises(ValueError, match="index of"):
        decode(jpeg_ops.decode_jpeg_batch_indexed, streams, layout, indexes)
    with pytest.raises(ValueError, match="indexes"):
        decode(jpeg_ops.decode_jpeg_batch_indexed, streams, layout, indexes[:-1])
