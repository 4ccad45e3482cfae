"""Baseline JPEG frames decoded on the device (csrc/jpeg.hip, `md2_jpeg_run`).

`parse_jpeg(data)` reads a file's headers on the host, in pure Python and without decoding
anything, and returns a `JpegStream` for the class of files the kernels take: one baseline
(SOF0) 8-bit frame of three YCbCr components sampled 4:4:4, 4:2:2 or 4:2:0, one scan, no
restart interval.  Anything else gives None and the caller decodes with PIL as before.

`decode_jpeg_batch(streams, out, offsets, device)` uploads the unstuffed entropy-coded
segments of a batch with their (deduplicated) tables in one pinned block and runs the
decoder: frame i lands in `out` as a tight (h, w, 3) image at byte `offsets[i]`, every byte
equal to `np.asarray(Image.open(path).convert("RGB"))`.  There is no CPU path: a non-CUDA
device is an error.

The other direction (csrc/jpegenc.hip, `md2_jpeg_encode`): `encode_jpeg_batch(frames,
quality, sampling)` encodes RGB frames of mixed sizes on the device and returns JpegStreams
with the quality's tables (`quality_tables`) and the standard Huffman tables, which the
decoder, the indexer and a pack take as they are; `jpeg_file_bytes(stream)` writes the file
around a stream on the host.  Every byte is what Pillow's `save(quality=, subsampling=)`
writes for the frame.
"""
from __future__ import annotations

import ctypes
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_DIM = 8192
SAMPLINGS = {((1, 1), (1, 1), (1, 1)): _lib.JPEG_444,
             ((2, 1), (1, 1), (1, 1)): _lib.JPEG_422,
             ((2, 2), (1, 1), (1, 1)): _lib.JPEG_420}

# zigzag position -> natural (row-major) index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
          41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

_STANDALONE = frozenset([0x01] + list(range(0xD0, 0xD8)))   # TEM, RSTn: no length field


class JpegStream:
    """What the device needs of one file.  quant[c]: component c's 64 quantisation steps in
    natural order; huff: {(cls, id): (counts[16], values)} with cls 0 = DC, 1 = AC; dc[c] /
    ac[c]: component c's table ids; data: the entropy-coded segment, unstuffed."""
    __slots__ = ("height", "width", "sampling", "factors", "quant", "huff", "dc", "ac", "data")

    def __init__(self, height, width, sampling, factors, quant, huff, dc, ac, data):
        self.height, self.width, self.sampling, self.factors = height, width, sampling, factors
        self.quant, self.huff, self.dc, self.ac, self.data = quant, huff, dc, ac, data

    @property
    def size(self) -> Tuple[int, int]:
        """(width, height), as PIL's Image.size."""
        return (self.width, self.height)


def unstuff(segment: bytes) -> bytes:
    """The entropy-coded bytes with every stuffed FF 00 turned back into FF."""
    return bytes(segment).replace(b"\xff\x00", b"\xff")


def entropy_segment(d: bytes, start: int) -> Optional[bytes]:
    """The entropy-coded segment that starts at byte `start`, unstuffed: up to the first
    FF xx with xx != 00, which must be the EOI (else None).  In numpy, whose loops run
    without the interpreter lock: this is the one step that touches every byte of the file,
    and the loader's threads do it side by side."""
    a = np.frombuffer(d, np.uint8, offset=start) if start < len(d) else np.zeros(0, np.uint8)
    ff = np.flatnonzero(a[:-1] == 0xFF)
    after = a[ff + 1]
    marker = np.flatnonzero(after)
    if marker.size == 0 or after[marker[0]] != 0xD9:
        return None
    end = int(ff[marker[0]])
    keep = np.ones(end, dtype=bool)
    keep[ff[:marker[0]] + 1] = False          # the zero of every FF 00 before the EOI
    return a[:end][keep].tobytes()


def _huffman_ok(counts: Sequence[int], nvalues: int) -> bool:
    """A table the canonical construction can hold: as many values as codes, at most 256,
    and no length oversubscribed (the all-ones code of the last length stays free)."""
    if sum(counts) != nvalues or nvalues > 256 or nvalues < 1:
        return False
    code = 0
    for length, n in enumerate(counts, 1):
        code += n
        if code > (1 << length) - (1 if n else 0):
            return False
        code <<= 1
    return True


def parse_jpeg(data) -> Optional[JpegStream]:
    """The description of a supported baseline JPEG file, or None (see the module text)."""
    try:
        return _parse(bytes(data) if not isinstance(data, bytes) else data)
    except (struct.error, IndexError, ValueError):
        return None


def _parse(d: bytes) -> Optional[JpegStream]:
    if len(d) < 4 or d[0:2] != b"\xff\xd8":
        return None
    pos = 2
    qtabs: Dict[int, Tuple[int, ...]] = {}
    huff: Dict[Tuple[int, int], Tuple[Tuple[int, ...], bytes]] = {}
    frame = None
    while True:
        if pos + 4 > len(d) or d[pos] != 0xFF:
            return None
        while d[pos + 1] == 0xFF:   # fill bytes before a marker
            pos += 1
            if pos + 4 > len(d):
                return None
        m = d[pos + 1]
        pos += 2
        if m in _STANDALONE or m == 0xD8 or m == 0xD9 or m == 0x00:
            return None             # a restart marker, a second SOI or an EOI before any scan
        (length,) = struct.unpack_from(">H", d, pos)
        if length < 2 or pos + length > len(d):
            return None
        seg = d[pos + 2:pos + length]
        if m == 0xC0:               # SOF0: the one baseline frame
            if frame is not None or len(seg) < 6:
                return None
            prec, h, w, nc = struct.unpack_from(">BHHB", seg, 0)
            if prec != 8 or nc != 3 or len(seg) != 6 + 3 * nc:
                return None
            if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
                return None
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(3)]
            frame = (h, w, comps)
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return None             # extended, progressive, lossless, arithmetic frames
        elif m == 0xCC:
            return None             # arithmetic conditioning
        elif m == 0xC4:             # DHT, possibly several tables
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = tuple(seg[i + 1:i + 17])
                if tc > 1 or th > 3 or len(counts) != 16:
                    return None
                n = sum(counts)
                vals = seg[i + 17:i + 17 + n]
                if len(vals) != n or not _huffman_ok(counts, n):
                    return None
                huff[(tc, th)] = (counts, bytes(vals))
                i += 17 + n
        elif m == 0xDB:             # DQT, possibly several tables
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq != 0 or tq > 3 or i + 65 > len(seg):
                    return None     # 16-bit tables belong to 12-bit files
                zz = seg[i + 1:i + 65]
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = zz[k]
                if min(nat) < 1:
                    return None
                qtabs[tq] = tuple(nat)
                i += 65
        elif m == 0xDD:             # DRI
            if len(seg) != 2 or seg != b"\x00\x00":
                return None
        elif m == 0xEE:             # APP14: an Adobe marker picks the colour transform
            if seg[:5] == b"Adobe":
                return None
        elif m == 0xDA:             # SOS
            if frame is None:
                return None
            break
        elif m == 0xDC or m == 0xDE or m == 0xDF:
            return None             # DNL, hierarchical
        pos += length
    h, w, comps = frame
    if len(seg) != 1 + 2 * 3 + 3 or seg[0] != 3:
        return None
    if (seg[7], seg[8], seg[9]) != (0, 63, 0):
        return None
    ids = [c[0] for c in comps]
    if len(set(ids)) != 3 or bytes(ids) == b"RGB":
        return None                 # libjpeg would take R, G, B ids for an RGB file
    dc, ac = [], []
    for i in range(3):              # the scan lists the components in frame order
        if seg[1 + 2 * i] != ids[i]:
            return None
        dc.append(seg[2 + 2 * i] >> 4)
        ac.append(seg[2 + 2 * i] & 15)
    factors = tuple((c[1], c[2]) for c in comps)
    sampling = SAMPLINGS.get(factors)
    if sampling is None:
        return None
    if any(c[3] not in qtabs for c in comps):
        return None
    if any((0, t) not in huff for t in dc) or any((1, t) not in huff for t in ac):
        return None
    body = entropy_segment(d, pos + length)
    if body is None:
        return None                 # cut before EOI, or a second scan / restart marker
    used = {(0, t): huff[(0, t)] for t in dc}
    used.update({(1, t): huff[(1, t)] for t in ac})
    return JpegStream(h, w, sampling, factors, tuple(qtabs[c[3]] for c in comps), used, tuple(dc), tuple(ac),
                      body)


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


class _Plan:
    """Per device: the C plan (workspace, descriptor ring), a small ring of pinned staging
    blocks with the events behind their uploads, the device copy of the block and the status
    words.  Everything grows to the largest batch seen and is then reused."""
    RING = 3

    def __init__(self, device: torch.device):
        self.device = device
        self.plan = None
        self.max_images = 0
        self.workspace = 0
        self.pinned: List[Optional[torch.Tensor]] = [None] * self.RING
        self.events: List[Optional[torch.cuda.Event]] = [None] * self.RING
        self.slot = 0
        self.staged: Optional[torch.Tensor] = None
        self.status: Optional[torch.Tensor] = None

    def reserve(self, n: int, workspace: int):
        if self.plan is not None and n <= self.max_images and workspace <= self.workspace:
            return
        L = _lib.lib()
        if self.plan is not None:
            L.md2_jpeg_plan_destroy(self.plan)   # waits for the work that uses it
            self.plan = None
        self.max_images = max(n, self.max_images)
        self.workspace = max(workspace + workspace // 8, self.workspace)
        with torch.cuda.device(self.device):
            self.plan = L.md2_jpeg_plan_create(self.max_images, self.workspace)
        if not self.plan:
            self.max_images = self.workspace = 0
            _lib.check(-1, "md2_jpeg_plan_create")
        self.status = torch.zeros(self.max_images, dtype=torch.int32, device=self.device)

    def stage(self, nbytes: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
        r = self.slot
        self.slot = (r + 1) % self.RING
        if self.events[r] is not None:
            self.events[r].synchronize()   # its upload has run (RING calls ago)
        if self.pinned[r] is None or self.pinned[r].numel() < nbytes:
            self.pinned[r] = torch.empty(nbytes + nbytes // 8, dtype=torch.uint8, pin_memory=True)
        if self.staged is None or self.staged.numel() < nbytes:
            self.staged = torch.empty(nbytes + nbytes // 8, dtype=torch.uint8, device=self.device)
        return self.pinned[r], self.staged, r

    def __del__(self):
        try:
            if self.plan is not None:
                _lib.lib().md2_jpeg_plan_destroy(self.plan)
        except Exception:
            pass


_plans: Dict[torch.device, _Plan] = {}


def _plan_for(device: torch.device) -> _Plan:
    p = _plans.get(device)
    if p is None:
        p = _plans[device] = _Plan(device)
    return p


def describe_batch(streams: Sequence[JpegStream], offsets: Sequence[int]):
    """The host side of a call: the md2_jpeg_image array, the deduplicated table bank
    (quantisation tables as uint16 in natural order, Huffman tables as counts + values) and
    the byte layout of the staging block: (images, quant_tables, huff_tables, stream_base,
    total_bytes), streams at 16-byte aligned offsets behind the tables."""
    n = len(streams)
    if n != len(offsets):
        raise ValueError(f"{n} streams but {len(offsets)} offsets")
    images = (_lib.JpegImage * max(n, 1))()
    quant: Dict[Tuple[int, ...], int] = {}
    huff: Dict[Tuple[Tuple[int, ...], bytes], int] = {}
    for i, s in enumerate(streams):
        im = images[i]
        im.height, im.width, im.sampling = s.height, s.width, s.sampling
        im.out_offset = int(offsets[i])
        im.stream_bytes = len(s.data)
        for c in range(3):
            im.quant[c] = quant.setdefault(s.quant[c], len(quant))
            im.dc[c] = huff.setdefault(s.huff[(0, s.dc[c])], len(huff))
            im.ac[c] = huff.setdefault(s.huff[(1, s.ac[c])], len(huff))
    if len(quant) > 255 or len(huff) > 255:
        raise ValueError("more than 255 distinct tables in one batch: decode it in parts")
    base = _align(len(quant) * _lib.JPEG_QUANT_BYTES + len(huff) * _lib.JPEG_HUFF_BYTES, 16)
    pos = 0
    for i, s in enumerate(streams):
        images[i].stream_offset = pos
        pos += _align(len(s.data), 16)
    return images, list(quant), list(huff), base, base + max(pos, 16)


def fill_staging(host: np.ndarray, streams, images, quant, huff, base: int):
    """The staging block of describe_batch's layout written into `host` (uint8)."""
    q = np.asarray(quant, dtype=np.uint16).reshape(-1)
    nq = q.size * 2
    host[:nq] = q.view(np.uint8)
    pos = nq
    for counts, vals in huff:
        host[pos:pos + 16] = counts
        host[pos + 16:pos + 16 + len(vals)] = np.frombuffer(vals, np.uint8)
        host[pos + 16 + len(vals):pos + _lib.JPEG_HUFF_BYTES] = 0
        pos += _lib.JPEG_HUFF_BYTES
    for i, s in enumerate(streams):
        o = base + images[i].stream_offset
        host[o:o + len(s.data)] = np.frombuffer(s.data, np.uint8)


def check_described(images, n: int, num_quant: int, num_huff: int, streams_bytes: int, out_bytes: int):
    """md2_jpeg_run's argument checks alone (host only): raises what it would refuse."""
    _lib.check(_lib.lib().md2_jpeg_check(images, n, num_quant, num_huff, streams_bytes, out_bytes), "md2_jpeg_check")


def run_staged(staged: torch.Tensor, images, n: int, num_quant: int, num_huff: int, base: int, total: int,
               out: torch.Tensor, device: torch.device) -> torch.Tensor:
    """The launches of a call whose staging block (describe_batch's layout, fill_staging's
    bytes) is already on its way to the device tensor `staged` on the current stream.
    Returns the plan's status words of the call (overwritten by the next call)."""
    L = _lib.lib()
    need = L.md2_jpeg_workspace_bytes(images, n)
    if need == 0:
        _lib.check(-1, "md2_jpeg_workspace_bytes")
    plan = _plan_for(device)
    with torch.cuda.device(device):
        plan.reserve(n, need)
        ptr = staged.data_ptr()
        bank = _lib.JpegBank(ptr, ptr + num_quant * _lib.JPEG_QUANT_BYTES, num_quant, num_huff)
        _lib.check(L.md2_jpeg_run(plan.plan, ptr + base, total - base, images, n, ctypes.byref(bank), out.data_ptr(),
                                  out.numel(), plan.status.data_ptr(), _lib.stream(device)), "md2_jpeg_run")
    return plan.status[:n]


def decode_jpeg_batch(streams: Sequence[JpegStream], out: torch.Tensor, offsets: Sequence[int], device=None,
                      check: bool = False) -> torch.Tensor:
    """Decodes `streams` into the uint8 device buffer `out`: frame i is the tight (h, w, 3)
    image at byte offsets[i] (a multiple of 16); no other byte of `out` is written.  One
    asynchronous upload of one pinned block (tables and streams), then the launches, on the
    current stream of `device`; nothing is allocated and nothing waits once the plan has
    grown to the batch's needs.  Returns the int32 status words of the call, one per stream,
    on the device (0 = decoded; they are the plan's and the next call overwrites them).
    check=True synchronises and raises a RuntimeError naming the first index whose status is
    not 0."""
    device = torch.device(device) if device is not None else (out.device if torch.is_tensor(out) else None)
    if device is None or device.type != "cuda" or not torch.is_tensor(out) or not out.is_cuda:
        raise RuntimeError("decode_jpeg_batch is GPU only (HIP kernels, no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if out.device != device or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor on {device}")
    n = len(streams)
    if n == 0:
        return torch.zeros(0, dtype=torch.int32, device=device)
    images, quant, huff, base, total = describe_batch(streams, offsets)
    check_described(images, n, len(quant), len(huff), total - base, out.numel())
    plan = _plan_for(device)
    with torch.cuda.device(device):
        pinned, staged, r = plan.stage(total)
        fill_staging(pinned.numpy(), streams, images, quant, huff, base)
        staged[:total].copy_(pinned[:total], non_blocking=True)
        if plan.events[r] is None:
            plan.events[r] = torch.cuda.Event()
        plan.events[r].record()
        status = run_staged(staged, images, n, len(quant), len(huff), base, total, out, device)
        if check:
            bad = torch.nonzero(status.cpu()).flatten().tolist()
            if bad:
                raise RuntimeError(f"decode_jpeg_batch: stream index {bad[0]} did not decode "
                                   f"(status {int(status[bad[0]])}); bad indices {bad}")
    return status


# ------------------------------------------------------------------ stored synchronisation indexes
# md2_jpeg_index / md2_jpeg_run_indexed (include/md2hot.h): an image's index is nsub uint64 entry
# states, then nsub uint32 first_block counts, zero padded to 16 bytes; here one uint8 array.
SUB_BITS = 1024
INDEX_ALIGN = 16


def index_nsub(stream_bytes: int) -> int:
    """Subsequences of a stream of `stream_bytes` bytes."""
    return max(-(-8 * int(stream_bytes) // SUB_BITS), 1)


def index_nbytes(stream_bytes: int) -> int:
    """Bytes of the index of a stream of `stream_bytes` bytes (md2_jpeg_index_bytes)."""
    return _align(12 * index_nsub(stream_bytes), INDEX_ALIGN)


def pack_index(states: Sequence[int], first_blocks: Sequence[int]) -> np.ndarray:
    """The index bytes of per-subsequence packed entry states (bit << 16 | block_in_mcu << 8 |
    zigzag) and first_block counts."""
    n = len(states)
    if n < 1 or n != len(first_blocks):
        raise ValueError(f"{n} states but {len(first_blocks)} first_block counts")
    out = np.zeros(_align(12 * n, INDEX_ALIGN), np.uint8)
    out[:8 * n] = np.asarray(states, dtype="<u8").view(np.uint8)
    out[8 * n:12 * n] = np.asarray(first_blocks, dtype="<u4").view(np.uint8)
    return out


def unpack_index(index: np.ndarray, stream_bytes: int) -> Tuple[np.ndarray, np.ndarray]:
    """(states uint64[nsub], first_blocks uint32[nsub]) of the index of a stream of `stream_bytes` bytes."""
    n = index_nsub(stream_bytes)
    raw = np.ascontiguousarray(index, dtype=np.uint8).reshape(-1)
    if raw.size != index_nbytes(stream_bytes):
        raise ValueError(f"an index of {raw.size} bytes for a stream of {stream_bytes} bytes (expected "
                         f"{index_nbytes(stream_bytes)})")
    return raw[:8 * n].view("<u8").copy(), raw[8 * n:12 * n].view("<u4").copy()


def _offset_array(values: Sequence[int]):
    return (ctypes.c_uint64 * max(len(values), 1))(*[int(v) for v in values])


def describe_batch_indexed(streams: Sequence[JpegStream], offsets: Sequence[int]):
    """describe_batch for md2_jpeg_run_indexed: every stream has its index directly behind it
    (16-byte aligned), so one contiguous range of the block is one frame.  Returns (images,
    index_offsets, quant_tables, huff_tables, stream_base, total_bytes)."""
    images, quant, huff, base, _ = describe_batch(streams, offsets)
    pos, ix = 0, []
    for i, s in enumerate(streams):
        images[i].stream_offset = pos
        pos += _align(len(s.data), INDEX_ALIGN)
        ix.append(pos)
        pos += index_nbytes(len(s.data))
    return images, _offset_array(ix), quant, huff, base, base + max(pos, 16)


def fill_staging_indexed(host: np.ndarray, streams, indexes, images, index_offsets, quant, huff, base: int):
    """The staging block of describe_batch_indexed's layout written into `host` (uint8)."""
    fill_staging(host, streams, images, quant, huff, base)
    for i, s in enumerate(streams):
        raw = np.ascontiguousarray(indexes[i], dtype=np.uint8).reshape(-1)
        if raw.size != index_nbytes(len(s.data)):
            raise ValueError(f"stream {i}: an index of {raw.size} bytes for {len(s.data)} stream bytes "
                             f"(expected {index_nbytes(len(s.data))})")
        o = base + index_offsets[i]
        host[o:o + raw.size] = raw


def check_described_indexed(images, index_offsets, n: int, num_quant: int, num_huff: int, streams_bytes: int,
                            out_bytes: int):
    """md2_jpeg_run_indexed's argument checks alone (host only): raises what it would refuse."""
    _lib.check(_lib.lib().md2_jpeg_check_indexed(images, index_offsets, n, num_quant, num_huff, streams_bytes,
                                                 out_bytes), "md2_jpeg_check_indexed")


def run_staged_indexed(staged: torch.Tensor, images, index_offsets, n: int, num_quant: int, num_huff: int, base: int,
                       total: int, out: torch.Tensor, device: torch.device) -> torch.Tensor:
    """run_staged for a block of describe_batch_indexed's layout (or the loader's packed one:
    tables, then records of stream + index): md2_jpeg_run_indexed's launches."""
    L = _lib.lib()
    need = L.md2_jpeg_workspace_bytes(images, n)
    if need == 0:
        _lib.check(-1, "md2_jpeg_workspace_bytes")
    plan = _plan_for(device)
    with torch.cuda.device(device):
        plan.reserve(n, need)
        ptr = staged.data_ptr()
        bank = _lib.JpegBank(ptr, ptr + num_quant * _lib.JPEG_QUANT_BYTES, num_quant, num_huff)
        _lib.check(L.md2_jpeg_run_indexed(plan.plan, ptr + base, total - base, images, index_offsets, n,
                                          ctypes.byref(bank), out.data_ptr(), out.numel(), plan.status.data_ptr(),
                                          _lib.stream(device)), "md2_jpeg_run_indexed")
    return plan.status[:n]


def _cuda_device(device, what: str) -> torch.device:
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"{what} is GPU only (HIP kernels, no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def index_jpeg_batch(streams: Sequence[JpegStream], device=None, check: bool = False) -> List[np.ndarray]:
    """The synchronisation index of every stream (md2_jpeg_index: the entropy decoder's
    fixed-point iteration alone, no frame decoded), as uint8 arrays of index_nbytes(len(
    s.data)) bytes each: what decode_jpeg_batch_indexed and pack.write_pack take.  One upload,
    one launch, one copy back; waits for the result.  check=True raises a RuntimeError for a
    stream that does not hold exactly its image's blocks."""
    device = _cuda_device(device, "index_jpeg_batch")
    n = len(streams)
    if n == 0:
        return []
    images, quant, huff, base, total = describe_batch(streams, [0] * n)
    sizes = [index_nbytes(len(s.data)) for s in streams]
    ix = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    index_offsets = _offset_array(ix[:-1].tolist())
    L = _lib.lib()
    need = L.md2_jpeg_workspace_bytes(images, n)
    if need == 0:
        _lib.check(-1, "md2_jpeg_workspace_bytes")
    plan = _plan_for(device)
    with torch.cuda.device(device):
        pinned, staged, r = plan.stage(total)
        fill_staging(pinned.numpy(), streams, images, quant, huff, base)
        staged[:total].copy_(pinned[:total], non_blocking=True)
        if plan.events[r] is None:
            plan.events[r] = torch.cuda.Event()
        plan.events[r].record()
        plan.reserve(n, need)
        dev_index = torch.empty(int(ix[-1]), dtype=torch.uint8, device=device)
        ptr = staged.data_ptr()
        bank = _lib.JpegBank(ptr, ptr + len(quant) * _lib.JPEG_QUANT_BYTES, len(quant), len(huff))
        _lib.check(L.md2_jpeg_index(plan.plan, ptr + base, total - base, images, index_offsets, n, ctypes.byref(bank),
                                    dev_index.data_ptr(), dev_index.numel(), plan.status.data_ptr(),
                                    _lib.stream(device)), "md2_jpeg_index")
        host = dev_index.cpu().numpy()          # waits for the launch
        if check:
            bad = torch.nonzero(plan.status[:n].cpu()).flatten().tolist()
            if bad:
                raise RuntimeError(f"index_jpeg_batch: stream index {bad[0]} does not hold its image's blocks "
                                   f"(status {int(plan.status[bad[0]])}); bad indices {bad}")
    return [host[ix[i]:ix[i + 1]].copy() for i in range(n)]


def decode_jpeg_batch_indexed(streams: Sequence[JpegStream], indexes: Sequence[np.ndarray], out: torch.Tensor,
                              offsets: Sequence[int], device=None, check: bool = False) -> torch.Tensor:
    """decode_jpeg_batch from stored indexes (index_jpeg_batch's, or a pack's): the same
    upload with every stream's index behind it, md2_jpeg_run_indexed's launches, the same
    bytes in `out` and the same status words; a stream whose index does not fit it reports
    JPEG_ST_INDEX, and the other frames of the batch are unaffected."""
    device = torch.device(device) if device is not None else (out.device if torch.is_tensor(out) else None)
    if device is None or device.type != "cuda" or not torch.is_tensor(out) or not out.is_cuda:
        raise RuntimeError("decode_jpeg_batch_indexed is GPU only (HIP kernels, no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if out.device != device or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor on {device}")
    n = len(streams)
    if n != len(indexes):
        raise ValueError(f"{n} streams but {len(indexes)} indexes")
    if n == 0:
        return torch.zeros(0, dtype=torch.int32, device=device)
    images, index_offsets, quant, huff, base, total = describe_batch_indexed(streams, offsets)
    check_described_indexed(images, index_offsets, n, len(quant), len(huff), total - base, out.numel())
    plan = _plan_for(device)
    with torch.cuda.device(device):
        pinned, staged, r = plan.stage(total)
        fill_staging_indexed(pinned.numpy(), streams, indexes, images, index_offsets, quant, huff, base)
        staged[:total].copy_(pinned[:total], non_blocking=True)
        if plan.events[r] is None:
            plan.events[r] = torch.cuda.Event()
        plan.events[r].record()
        status = run_staged_indexed(staged, images, index_offsets, n, len(quant), len(huff), base, total, out, device)
        if check:
            bad = torch.nonzero(status.cpu()).flatten().tolist()
            if bad:
                raise RuntimeError(f"decode_jpeg_batch_indexed: stream index {bad[0]} did not decode "
                                   f"(status {int(status[bad[0]])}); bad indices {bad}")
    return status


# ------------------------------------------------------------------ encoding (csrc/jpegenc.hip)
# The base quantisation tables of ITU-T T.81 Annex K (K.1 luma, K.2 chroma), natural order.
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# The four Huffman tables of Annex K (K.3 to K.6) as a DHT segment lists them: the only ones
# the encoder writes.  {(class, id): (counts[16], values)}, class 0 = DC, id 0 = luma.
STD_HUFF = {
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a34"
        "35363738393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a9293949596"
        "9798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1"
        "f2f3f4f5f6f7f8f9fa")),
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a26272829"
        "2a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a929394"
        "95969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9ea"
        "f2f3f4f5f6f7f8f9fa")),
}

SAMPLING_NAMES = {"4:4:4": _lib.JPEG_444, "444": _lib.JPEG_444, "4:2:2": _lib.JPEG_422, "422": _lib.JPEG_422,
                  "4:2:0": _lib.JPEG_420, "420": _lib.JPEG_420}
_FACTORS = {v: k for k, v in SAMPLINGS.items()}


def sampling_class(sampling) -> int:
    """JPEG_444 / 422 / 420 from "4:2:0", "420", 420 or the class itself."""
    if isinstance(sampling, int) and sampling in _FACTORS:
        return sampling
    try:
        return SAMPLING_NAMES[str(sampling)]
    except KeyError:
        raise ValueError(f"unknown sampling {sampling!r} (4:4:4, 4:2:2 or 4:2:0)") from None


def quality_tables(quality: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(luma, chroma) quantisation tables of a quality 1..100 as libjpeg makes them, natural
    order: the base tables scaled by 5000 / quality below 50 and 200 - 2 quality from 50 on,
    (base * scale + 50) / 100 clipped to 1..255."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality} outside 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(max((b * scale + 50) // 100, 1), 255) for b in base) for base in (BASE_LUMA, BASE_CHROMA))


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_file_bytes(stream: JpegStream) -> bytes:
    """The JFIF file of a stream, written as Pillow (libjpeg) writes one: SOI, APP0 JFIF 1.01
    (no units, density 1 x 1), DQT 0 and 1 in zigzag order, SOF0 (components 1, 2, 3, tables
    0, 1, 1), DHT DC0, AC0, DC1, AC1, SOS, the data with every FF stuffed to FF 00, EOI.  Host
    only.  A stream this layout cannot hold is refused: luma factors other than 1x1 / 2x1 /
    2x2 over 1x1 chroma, or chroma components with different tables."""
    factors = tuple(tuple(f) for f in stream.factors)
    if factors not in SAMPLINGS:
        raise ValueError(f"jpeg_file_bytes: sampling factors {factors} (luma 1x1, 2x1 or 2x2 over 1x1 chroma)")
    quant = [tuple(int(v) for v in q) for q in stream.quant]
    if quant[1] != quant[2]:
        raise ValueError("jpeg_file_bytes: the chroma components use different quantisation tables")
    tabs = []
    for cls, ids in ((0, stream.dc), (1, stream.ac)):
        if stream.huff[(cls, ids[1])] != stream.huff[(cls, ids[2])]:
            raise ValueError("jpeg_file_bytes: the chroma components use different Huffman tables")
        tabs.append([stream.huff[(cls, ids[0])], stream.huff[(cls, ids[1])]])
    if any(len(q) != 64 or min(q) < 1 or max(q) > 255 for q in quant):
        raise ValueError("jpeg_file_bytes: a quantisation table is not 64 values of 1..255")
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for tid, q in ((0, quant[0]), (1, quant[1])):
        out.append(_segment(0xDB, bytes([tid]) + bytes(q[ZIGZAG[k]] for k in range(64))))
    sof = struct.pack(">BHHB", 8, stream.height, stream.width, 3)
    for c in range(3):
        sof += bytes([c + 1, factors[c][0] << 4 | factors[c][1], 0 if c == 0 else 1])
    out.append(_segment(0xC0, sof))
    for tid in (0, 1):
        for cls in (0, 1):
            counts, vals = tabs[cls][tid]
            out.append(_segment(0xC4, bytes([cls << 4 | tid]) + bytes(counts) + bytes(vals)))
    out.append(_segment(0xDA, b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"))
    out.append(bytes(stream.data).replace(b"\xff", b"\xff\x00"))
    out.append(b"\xff\xd9")
    return b"".join(out)


def standard_stream(height: int, width: int, sampling: int, quality: int, data: bytes) -> JpegStream:
    """The JpegStream of an encoded frame: the quality's tables, the standard Huffman tables."""
    luma, chroma = quality_tables(quality)
    return JpegStream(height, width, sampling, _FACTORS[sampling], (luma, chroma, chroma), dict(STD_HUFF),
                      (0, 1, 1), (0, 1, 1), data)


def _per_image(value, n: int, what: str) -> list:
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{len(value)} {what} values for {n} frames")
        return list(value)
    return [value] * n


def encode_bound(height: int, width: int, sampling: int) -> int:
    """md2_jpeg_encode_bound: a capacity no stream of that geometry exceeds (208 bytes per block)."""
    need = _lib.lib().md2_jpeg_encode_bound(int(height), int(width), int(sampling))
    if need == 0:
        _lib.check(-1, "md2_jpeg_encode_bound")
    return need


def describe_encode(shapes: Sequence[Tuple[int, int]], samplings: Sequence[int], qualities: Sequence[int],
                    in_offsets: Sequence[int], out_offsets: Optional[Sequence[int]] = None,
                    capacities: Optional[Sequence[int]] = None):
    """The host side of an encode call: the md2_jpegenc_image array, the deduplicated bank of
    quantisation tables (natural order) and the bytes of `out` the ranges need: (images,
    quant_tables, out_bytes).  Without out_offsets every image gets md2_jpeg_encode_bound
    bytes at the next multiple of 16."""
    n = len(shapes)
    images = (_lib.JpegEncImage * max(n, 1))()
    quant: Dict[Tuple[int, ...], int] = {}
    pos = 0
    for i, (h, w) in enumerate(shapes):
        im = images[i]
        im.height, im.width, im.sampling = int(h), int(w), int(samplings[i])
        im.in_offset = int(in_offsets[i])
        luma, chroma = quality_tables(qualities[i])
        im.quant[0] = quant.setdefault(luma, len(quant))
        im.quant[1] = quant.setdefault(chroma, len(quant))
        if out_offsets is None:
            im.out_offset, im.out_capacity = pos, encode_bound(h, w, im.sampling)
        else:
            im.out_offset, im.out_capacity = int(out_offsets[i]), int(capacities[i])
        pos = max(pos, _align(im.out_offset + im.out_capacity, 16))
    if len(quant) > 256:
        raise ValueError("more than 256 distinct quantisation tables in one batch: encode it in parts")
    return images, list(quant), max(pos, 16)


def check_encode(images, n: int, num_quant: int, in_bytes: int, out_bytes: int):
    """md2_jpeg_encode's argument checks alone (host only): raises what it would refuse."""
    _lib.check(_lib.lib().md2_jpeg_encode_check(images, n, num_quant, in_bytes, out_bytes), "md2_jpeg_encode_check")


def encode_tables_bytes(n: int, num_quant: int) -> int:
    """Bytes of the block run_encode reads its tables from: the image array, then the bank."""
    return _align(n * ctypes.sizeof(_lib.JpegEncImage), 16) + num_quant * _lib.JPEG_QUANT_BYTES


def fill_encode_tables(host: np.ndarray, images, n: int, quant):
    """The image array and the quantisation bank written into `host` (uint8) in
    encode_tables_bytes's layout."""
    nb = n * ctypes.sizeof(_lib.JpegEncImage)
    host[:nb] = np.frombuffer(images, np.uint8, nb)
    q0 = _align(nb, 16)
    host[nb:q0] = 0
    host[q0:q0 + len(quant) * _lib.JPEG_QUANT_BYTES] = np.asarray(quant, dtype=np.uint16).reshape(-1).view(np.uint8)


def run_encode(tables: torch.Tensor, frames: torch.Tensor, images, n: int, num_quant: int, out: torch.Tensor,
               device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """The launches of an encode call whose tables (fill_encode_tables's bytes, 16-byte aligned)
    and frames are on the device or on their way there on the current stream.  Returns
    (stream_bytes, status), uint32 values in int32 tensors of n on the device."""
    L = _lib.lib()
    need = L.md2_jpeg_encode_workspace_bytes(images, n)
    if need == 0:
        _lib.check(-1, "md2_jpeg_encode_workspace_bytes")
    with torch.cuda.device(device):
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        result = torch.empty((2, n), dtype=torch.int32, device=device)
        q0 = _align(n * ctypes.sizeof(_lib.JpegEncImage), 16)
        _lib.check(L.md2_jpeg_encode(frames.data_ptr(), frames.numel(), images, tables.data_ptr(), n,
                                     tables.data_ptr() + q0, num_quant, out.data_ptr(), out.numel(),
                                     workspace.data_ptr(), need, result[0].data_ptr(), result[1].data_ptr(),
                                     _lib.stream(device)), "md2_jpeg_encode")
    return result[0], result[1]


def encode_jpeg_batch(frames, quality=92, sampling="4:2:0", device=None, check: bool = False, offsets=None,
                      sizes=None, fill=None, pool=None) -> List[JpegStream]:
    """Encodes a batch of RGB frames as baseline JPEG on the device (md2_jpeg_encode): every
    stream's data, tables and jpeg_file_bytes output are what Pillow's save(quality=...,
    subsampling=...) writes for the frame.  `frames`: a list of (h, w, 3) uint8 arrays or
    tensors of mixed sizes, or one flat uint8 device tensor with `offsets` (bytes) and `sizes`
    ((h, w) each) of the tight frames in it.  quality and sampling: one value, or one per
    frame.  Host frames travel in one pinned block with the tables (one upload); then the
    launches; then the lengths and status words come back, and the streams in one copy of
    exactly their bytes.  The streams carry the quality's tables and the standard Huffman
    tables, so decode_jpeg_batch, index_jpeg_batch and pack records take them as they are.
    check=True raises a RuntimeError naming the first frame whose status is not 0 (such a
    stream has empty data).  With `fill`, `frames` is a list of (h, w) sizes and fill(i, dest)
    writes frame i into dest, an (h, w, 3) uint8 view of the pinned block (through pool.map if
    a thread pool is given): a decoder's output lands in pinned memory without a copy of the
    list.  There is no CPU path."""
    device = _cuda_device(device, "encode_jpeg_batch")
    flat = torch.is_tensor(frames) and offsets is not None
    if flat:
        if sizes is None or len(sizes) != len(offsets):
            raise ValueError("a flat frame buffer needs as many sizes as offsets")
        if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 1 or not frames.is_contiguous():
            raise ValueError("a flat frame buffer must be a contiguous 1-D uint8 device tensor")
        shapes = [(int(h), int(w)) for h, w in sizes]
        in_offsets = [int(o) for o in offsets]
        arrays = None
    elif fill is not None:
        arrays = None
        shapes = [(int(h), int(w)) for h, w in frames]
    else:
        arrays = []
        for f in frames:
            a = f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"a frame must be (h, w, 3) uint8, not {a.dtype} {a.shape}")
            arrays.append(np.ascontiguousarray(a))
        shapes = [a.shape[:2] for a in arrays]
    n = len(shapes)
    if n == 0:
        return []
    samplings = [sampling_class(s) for s in _per_image(sampling, n, "sampling")]
    qualities = [int(q) for q in _per_image(quality, n, "quality")]
    tables_bytes = _align(encode_tables_bytes(n, 2 * n), 16)   # room for every table before they are deduplicated
    if not flat:
        in_offsets, pos = [], 0
        for h, w in shapes:
            in_offsets.append(pos)
            pos += _align(h * w * 3, 16)
        frames_bytes = max(pos, 16)
    images, quant, out_bytes = describe_encode(shapes, samplings, qualities, in_offsets)
    with torch.cuda.device(device):
        total = tables_bytes + (0 if flat else frames_bytes)
        pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        fill_encode_tables(host, images, n, quant)
        if fill is not None:
            def one(i):
                h, w = shapes[i]
                o = tables_bytes + in_offsets[i]
                fill(i, host[o:o + h * w * 3].reshape(h, w, 3))
            list(pool.map(one, range(n)) if pool is not None else map(one, range(n)))
        elif not flat:
            for a, o in zip(arrays, in_offsets):
                host[tables_bytes + o:tables_bytes + o + a.size] = a.reshape(-1)
        staged = torch.empty(total, dtype=torch.uint8, device=device)
        staged.copy_(pinned, non_blocking=True)
        source = frames if flat else staged[tables_bytes:]
        check_encode(images, n, len(quant), source.numel(), out_bytes)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=device)
        lengths, status = run_encode(staged, source, images, n, len(quant), out, device)
        result = torch.stack([lengths, status]).cpu().numpy().astype(np.int64) & 0xFFFFFFFF   # waits for the launches
        lens = [0 if result[1, i] else int(result[0, i]) for i in range(n)]
        bad = np.flatnonzero(result[1]).tolist()
        if check and bad:
            raise RuntimeError(f"encode_jpeg_batch: frame index {bad[0]} did not encode (status "
                               f"{int(result[1, bad[0]])}); bad indices {bad}")
        parts = [out[images[i].out_offset:images[i].out_offset + lens[i]] for i in range(n)]
        data = torch.cat(parts).cpu().numpy().tobytes()
    streams, pos = [], 0
    for i in range(n):
        streams.append(standard_stream(shapes[i][0], shapes[i][1], samplings[i], qualities[i], data[pos:pos + lens[i]]))
        pos += lens[i]
    return streams
