"""The device JPEG encoder (csrc/jpegenc.hip, jpeg_ops.encode_jpeg_batch) against Pillow, byte
for byte and with no tolerance: the entropy-coded segment, both quantisation tables and the
complete file of every case of tests/jpeg_encode_case.py (three samplings x four qualities on
sizes with partial MCUs, dummy blocks, one- and two-sample chroma planes and the h % 16 == 8
bottom rule; a flat frame whose six blocks share two words; noise at quality 100 with FF bytes; runs of 16
zeros; one KITTI-sized frame).  All cases are encoded in a few calls and shared by the tests."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_encode_case as ec
from monodepth2_amd import _lib, jpeg_ops

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 48          # canary bytes in front of, between and behind the output ranges


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def encoded(device):
    """name -> JpegStream, every case encoded on the device in one call of mixed sizes,
    samplings and qualities."""
    names = list(ec.CASES)
    streams = jpeg_ops.encode_jpeg_batch([ec.frame(n) for n in names], quality=[ec.CASES[n][5] for n in names],
                                         sampling=[ec.CASES[n][4] for n in names], device=device, check=True)
    return dict(zip(names, streams))


@pytest.mark.parametrize("name", list(ec.CASES))
def test_equal_to_pillow(encoded, name):
    s = encoded[name]
    ref = ec.pillow_file(name)
    p = jpeg_ops.parse_jpeg(ref)
    assert (s.height, s.width, s.sampling, s.factors) == (p.height, p.width, p.sampling, p.factors)
    assert s.quant == p.quant
    assert s.huff == p.huff and s.dc == p.dc and s.ac == p.ac
    assert len(s.data) == len(p.data), (len(s.data), len(p.data))
    assert s.data == p.data
    assert jpeg_ops.jpeg_file_bytes(s) == ref


def test_stream_has_ff_bytes(encoded):
    """the noise case is there for the stuffing: its stream must hold FF bytes"""
    assert b"\xff" in encoded["noise_64x96_444_q100"].data
    assert len(encoded["flat_16x16_420_q75"].data) <= 8   # six blocks share two words


def test_default_save(device):
    """Pillow's defaults are quality 75, 4:2:0: what infer writes"""
    a = ec.frame("grid_37x53_420_q75")
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG")
    (s,) = jpeg_ops.encode_jpeg_batch([a], quality=75, sampling="4:2:0", device=device, check=True)
    assert jpeg_ops.jpeg_file_bytes(s) == buf.getvalue()


def test_flat_device_buffer(device, encoded):
    """frames already on the device, addressed by offsets and sizes (unaligned offsets too)"""
    names = ("grid_17x33_422_q92", "grid_9x3_420_q30", "grid_37x53_444_q100")
    offsets, pos, parts = [], 5, [np.zeros(5, np.uint8)]
    for n in names:
        offsets.append(pos)
        parts.append(ec.frame(n).reshape(-1))
        pos += parts[-1].size
    buf = torch.from_numpy(np.concatenate(parts)).to(device)
    streams = jpeg_ops.encode_jpeg_batch(buf, quality=[ec.CASES[n][5] for n in names],
                                         sampling=[ec.CASES[n][4] for n in names], device=device, check=True,
                                         offsets=offsets, sizes=[ec.frame(n).shape[:2] for n in names])
    for n, s in zip(names, streams):
        assert s.data == encoded[n].data, n


def _mixed_call(device, short=None):
    """One md2_jpeg_encode call on the MIXED cases with canary bytes around every output
    range.  short: index of an image whose capacity is one byte less than its stream.
    Returns (out bytes, lengths, status, images)."""
    names = ec.MIXED
    frames = [ec.frame(n) for n in names]
    shapes = [f.shape[:2] for f in frames]
    samplings = [jpeg_ops.sampling_class(ec.CASES[n][4]) for n in names]
    qualities = [ec.CASES[n][5] for n in names]
    want = [len(jpeg_ops.parse_jpeg(ec.pillow_file(n)).data) for n in names]
    in_offsets, out_offsets, caps, pos, opos = [], [], [], 0, GAP
    for i, f in enumerate(frames):
        in_offsets.append(pos)
        pos += f.size
        cap = want[i] - 1 if i == short else want[i]     # exactly the stream: not a byte to spare
        out_offsets.append(opos)
        caps.append(cap)
        opos = (opos + cap + GAP + 15) // 16 * 16
    images, quant, _ = jpeg_ops.describe_encode(shapes, samplings, qualities, in_offsets, out_offsets, caps)
    n = len(names)
    tb = (jpeg_ops.encode_tables_bytes(n, len(quant)) + 15) // 16 * 16
    host = np.zeros(tb + pos, np.uint8)
    jpeg_ops.fill_encode_tables(host, images, n, quant)
    host[tb:] = np.concatenate([f.reshape(-1) for f in frames])
    staged = torch.from_numpy(host).to(device)
    out = torch.full((opos + GAP,), CANARY, dtype=torch.uint8, device=device)
    jpeg_ops.check_encode(images, n, len(quant), pos, out.numel())
    lengths, status = jpeg_ops.run_encode(staged, staged[tb:], images, n, len(quant), out, device)
    return out.cpu().numpy(), lengths.cpu().numpy(), status.cpu().numpy(), images


def _check_mixed(out, lengths, status, images, short=None):
    owned = np.zeros(out.size, bool)
    for i, name in enumerate(ec.MIXED):
        want = jpeg_ops.parse_jpeg(ec.pillow_file(name)).data
        o, cap = images[i].out_offset, images[i].out_capacity
        owned[o:o + cap] = True
        assert lengths[i] == len(want), name
        if i == short:
            assert status[i] == _lib.JPEGENC_ST_SPACE, name
        else:
            assert status[i] == 0, name
            assert out[o:o + len(want)].tobytes() == want, name
    assert (out[~owned] == CANARY).all(), "a byte outside every output range was written"


def test_mixed_batch_with_canaries(device):
    """all three samplings and six sizes in one call, every range exactly as long as its
    stream: no image disturbs a neighbour, nothing outside a range is written"""
    assert len({ec.CASES[n][4] for n in ec.MIXED}) == 3 and len({ec.CASES[n][1:3] for n in ec.MIXED}) >= 6
    _check_mixed(*_mixed_call(device))


@pytest.mark.parametrize("short", [0, 4, len(ec.MIXED) - 1])
def test_capacity_one_byte_short(device, short):
    """that image alone reports MD2_JPEGENC_ST_SPACE; the canaries stay intact"""
    _check_mixed(*_mixed_call(device, short=short), short=short)


def test_two_runs_bit_equal(device):
    a = _mixed_call(device)
    b = _mixed_call(device)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_round_trip(device, encoded):
    """decode_jpeg_batch(encode_jpeg_batch(x)) equals Pillow's decode of Pillow's file"""
    names = list(ec.MIXED) + ["kitti_375x1242_420_q92", "textured_64x96_420_q30"]
    streams = [encoded[n] for n in names]
    offsets, pos = [], 0
    for s in streams:
        offsets.append(pos)
        pos += (s.height * s.width * 3 + 15) // 16 * 16
    out = torch.zeros(pos, dtype=torch.uint8, device=device)
    jpeg_ops.decode_jpeg_batch(streams, out, offsets, device=device, check=True)
    got = out.cpu().numpy()
    for n, s, o in zip(names, streams, offsets):
        ref = np.asarray(Image.open(io.BytesIO(ec.pillow_file(n))).convert("RGB"))
        assert np.array_equal(got[o:o + ref.size].reshape(ref.shape), ref), n


def test_index_takes_encoded_streams(device, encoded):
    """index_jpeg_batch accepts the encoder's streams as they are (what a pack stores)"""
    names = ("kitti_375x1242_420_q92", "grid_24x40_420_q92")
    ix = jpeg_ops.index_jpeg_batch([encoded[n] for n in names], device=device, check=True)
    for n, a in zip(names, ix):
        assert a.size == jpeg_ops.index_nbytes(len(encoded[n].data))


def test_struct_size():
    assert ctypes.sizeof(_lib.JpegEncImage) == 40
