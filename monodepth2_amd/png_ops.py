"""8-bit RGB PNG frames decoded on the device (csrc/png.hip, `md2_png_run`).

`parse_png(data)` reads a file's chunks on the host, in pure Python and without decoding
anything, and returns a `PngStream` for the class of files the kernels take: the signature,
IHDR first (1..8192 x 1..8192, bit depth 8, colour type 2, not interlaced), one run of IDAT
chunks whose payloads form a zlib stream (CM 8, window at most 32 KiB, no preset dictionary),
IEND, every chunk's CRC right.  Ancillary chunks are skipped (a tRNS chunk on an RGB file does
not change Pillow's convert("RGB")).  Anything else gives None and the caller decodes with
PIL as before: gray, palette, alpha, 16-bit, interlaced, APNG, a bad CRC, a missing IEND, a
file that is not PNG.

`decode_png_batch(streams, out, offsets, device)` uploads the deflate streams of a batch in
one pinned block and runs the decoder (inflate, then unfilter with the Adler-32 check): frame
i lands in `out` as a tight (h, w, 3) image at byte `offsets[i]`, every byte equal to
`np.asarray(Image.open(path).convert("RGB"))`.  There is no CPU path: a non-CUDA device is an
error.

The indexed decoder (`md2_png_run_indexed`) inflates the segments of a stream
at the same time from an index of where they start.  `index_png_batch(streams, segment_bytes)`
finds the indexes on the device (once: a frame pack keeps them behind the streams),
`index_nbytes(h, w, segment_bytes)` is an index's size (fixed per geometry), and
`decode_png_batch_indexed(streams, indexes, out, offsets)` is `decode_png_batch` from them:
the same bytes and status words, or `_lib.PNG_ST_INDEX` for an index that does not fit.
"""
from __future__ import annotations

import ctypes
import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_DIM = 8192
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_KNOWN_CRITICAL = (b"IHDR", b"PLTE", b"IDAT", b"IEND")

STATUS_NAMES = ((_lib.PNG_ST_BLOCK, "a block type or stored length zlib refuses"),
                (_lib.PNG_ST_CODE, "a Huffman code set or code zlib refuses"),
                (_lib.PNG_ST_END, "the stream ends before the image is complete"),
                (_lib.PNG_ST_DIST, "a match distance before the first byte"),
                (_lib.PNG_ST_FILTER, "a filter byte above 4"),
                (_lib.PNG_ST_ADLER, "the Adler-32 trailer does not fit the scanlines"),
                (_lib.PNG_ST_INDEX, "the segment index does not fit the stream"))
SEGMENT_BYTES = 16384   # the default S of an index


def status_text(word: int) -> str:
    """What the bits of a status word say."""
    return "; ".join(text for bit, text in STATUS_NAMES if word & bit) or "decoded"


class PngStream:
    """What the device needs of one file.  data: the raw deflate stream followed by the 4
    bytes of the Adler-32 trailer (the zlib stream of the IDAT chunks without its 2-byte
    header)."""
    __slots__ = ("height", "width", "data")

    def __init__(self, height, width, data):
        self.height, self.width, self.data = height, width, data

    @property
    def size(self) -> Tuple[int, int]:
        """(width, height), as PIL's Image.size."""
        return (self.width, self.height)


def parse_png(data) -> Optional[PngStream]:
    """The description of a supported PNG file, or None (see the module text)."""
    try:
        return _parse(bytes(data) if not isinstance(data, bytes) else data)
    except (struct.error, IndexError, ValueError, TypeError):
        return None


def _parse(d: bytes) -> Optional[PngStream]:
    if len(d) < 8 + 25 or d[:8] != SIGNATURE:
        return None
    view = memoryview(d)
    pos, size, idat, state = 8, None, [], 0      # state: 0 before IDAT, 1 inside the run, 2 behind it
    while True:
        if pos + 12 > len(d):
            return None                           # no IEND
        (length,) = struct.unpack_from(">I", d, pos)
        kind = d[pos + 4:pos + 8]
        end = pos + 8 + length
        if end + 4 > len(d):
            return None
        (crc,) = struct.unpack_from(">I", d, end)
        if zlib.crc32(view[pos + 4:end]) != crc:  # releases the interpreter lock
            return None
        if size is None:
            if kind != b"IHDR" or length != 13:
                return None
            w, h, depth, colour, compression, filt, interlace = struct.unpack_from(">IIBBBBB", d, pos + 8)
            if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
                return None
            if (depth, colour, compression, filt, interlace) != (8, 2, 0, 0, 0):
                return None
            size = (h, w)
        elif kind == b"IHDR":
            return None
        elif kind == b"IDAT":
            if state == 2:
                return None                       # a second run of IDAT chunks
            state = 1
            if length:
                idat.append(view[pos + 8:end])
        elif kind == b"IEND":
            break
        else:
            if state == 1:
                state = 2
            if kind in (b"acTL", b"fcTL", b"fdAT"):
                return None                       # APNG
            if not (kind[0] & 0x20) and kind not in _KNOWN_CRITICAL:
                return None                       # a critical chunk this reader does not know
        pos = end + 4
    if state == 0:
        return None
    z = b"".join(idat)
    if len(z) < 2 + 1 + 4:
        return None
    cmf, flg = z[0], z[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 0x20 or (cmf << 8 | flg) % 31:
        return None
    return PngStream(size[0], size[1], z[2:])


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


IMAGE_BYTES = ctypes.sizeof(_lib.PngImage)


def describe_png_batch(streams: Sequence[PngStream], offsets: Sequence[int]):
    """The host side of a call: the md2_png_image array and the byte layout of the staging
    block: (images, stream_base, total_bytes).  The block starts with the image array (the
    kernels read their copy of it there), the streams follow at 16-byte aligned offsets from
    stream_base."""
    n = len(streams)
    if n != len(offsets):
        raise ValueError(f"{n} streams but {len(offsets)} offsets")
    images = (_lib.PngImage * max(n, 1))()
    pos = 0
    for i, s in enumerate(streams):
        im = images[i]
        im.height, im.width = s.height, s.width
        im.out_offset = int(offsets[i])
        im.stream_offset, im.stream_bytes = pos, len(s.data)
        pos += _align(len(s.data), 16)
    base = _align(n * IMAGE_BYTES, 16)
    return images, base, base + max(pos, 16)


def fill_png_staging(host: np.ndarray, streams, images, base: int):
    """The staging block of describe_png_batch's layout written into `host` (uint8)."""
    nb = len(streams) * IMAGE_BYTES
    host[:nb] = np.frombuffer(images, np.uint8, nb)
    host[nb:base] = 0
    for i, s in enumerate(streams):
        o = base + images[i].stream_offset
        host[o:o + len(s.data)] = np.frombuffer(s.data, np.uint8)


def check_png_described(images, n: int, streams_bytes: int, out_bytes: int):
    """md2_png_run's argument checks alone (host only): raises what it would refuse."""
    _lib.check(_lib.lib().md2_png_check(images, n, streams_bytes, out_bytes), "md2_png_check")


def check_segment_bytes(segment_bytes: int) -> int:
    s = int(segment_bytes)
    if not 1024 <= s <= 32768 or s & (s - 1):
        raise ValueError(f"segment_bytes must be a power of two in 1024..32768, not {segment_bytes}")
    return s


def index_nbytes(height: int, width: int, segment_bytes: int = SEGMENT_BYTES) -> int:
    """The bytes of the index of a height x width frame for segment_bytes (md2_png_index_bytes):
    a 16-byte header and height * (1 + 3 width) // segment_bytes + 1 entries of 24 bytes,
    rounded up to 16."""
    s = check_segment_bytes(segment_bytes)
    if not (1 <= height <= MAX_DIM and 1 <= width <= MAX_DIM):
        raise ValueError(f"height and width must be 1..{MAX_DIM}, not {height} x {width}")
    cap = height * (1 + 3 * width) // s + 1
    return _align(_lib.PNG_INDEX_HEADER_BYTES + _lib.PNG_INDEX_ENTRY_BYTES * cap, 16)


def describe_png_batch_indexed(streams: Sequence[PngStream], indexes, offsets: Sequence[int], segment_bytes: int):
    """describe_png_batch for md2_png_run_indexed: (images, index_offsets, stream_base,
    total_bytes).  The block starts with the image array, the uint64 index offsets follow
    (at len(streams) * IMAGE_BYTES), then from stream_base each stream, zeros to 16 and its
    index: the bytes of a pack record."""
    n = len(streams)
    if n != len(offsets) or n != len(indexes):
        raise ValueError(f"{n} streams but {len(indexes)} indexes and {len(offsets)} offsets")
    images = (_lib.PngImage * max(n, 1))()
    index_offsets = (ctypes.c_uint64 * max(n, 1))()
    pos = 0
    for i, s in enumerate(streams):
        want = index_nbytes(s.height, s.width, segment_bytes)
        if len(indexes[i]) != want:
            raise ValueError(f"stream {i}: an index of {len(indexes[i])} bytes for a {s.height} x {s.width} frame "
                             f"(expected {want} at segment_bytes {segment_bytes})")
        im = images[i]
        im.height, im.width = s.height, s.width
        im.out_offset = int(offsets[i])
        im.stream_offset, im.stream_bytes = pos, len(s.data)
        index_offsets[i] = pos + _align(len(s.data), 16)
        pos += _align(len(s.data), 16) + want
    base = _align(n * (IMAGE_BYTES + 8), 16)
    return images, index_offsets, base, base + max(pos, 16)


def fill_png_staging_indexed(host: np.ndarray, streams, indexes, images, index_offsets, base: int):
    """The staging block of describe_png_batch_indexed's layout written into `host` (uint8)."""
    n = len(streams)
    nb = n * IMAGE_BYTES
    host[:nb] = np.frombuffer(images, np.uint8, nb)
    host[nb:nb + 8 * n] = np.frombuffer(index_offsets, np.uint8, 8 * n)
    host[nb + 8 * n:base] = 0
    for i, s in enumerate(streams):
        o = base + images[i].stream_offset
        host[o:o + len(s.data)] = np.frombuffer(s.data, np.uint8)
        host[o + len(s.data):base + index_offsets[i]] = 0
        o = base + index_offsets[i]
        host[o:o + len(indexes[i])] = np.frombuffer(indexes[i], np.uint8)


def check_png_described_indexed(images, index_offsets, n: int, segment_bytes: int, streams_bytes: int,
                                out_bytes: int):
    """md2_png_run_indexed's argument checks alone (host only): raises what it would refuse."""
    _lib.check(_lib.lib().md2_png_check_indexed(images, index_offsets, n, int(segment_bytes), streams_bytes,
                                                out_bytes), "md2_png_check_indexed")


class _Plan:
    """Per device: the workspace and the status words, which grow to the largest batch seen,
    and a small ring of pinned staging blocks with the events behind their uploads."""
    RING = 3

    def __init__(self, device: torch.device):
        self.device = device
        self.workspace: Optional[torch.Tensor] = None
        self.status: Optional[torch.Tensor] = None
        self.pinned: List[Optional[torch.Tensor]] = [None] * self.RING
        self.events: List[Optional[torch.cuda.Event]] = [None] * self.RING
        self.slot = 0
        self.staged: Optional[torch.Tensor] = None

    def reserve(self, n: int, workspace: int):
        if self.workspace is None or self.workspace.numel() < workspace:
            self.workspace = torch.empty(workspace + workspace // 8, dtype=torch.uint8, device=self.device)
        if self.status is None or self.status.numel() < n:
            self.status = torch.zeros(n, dtype=torch.int32, device=self.device)

    def stage(self, nbytes: int):
        r = self.slot
        self.slot = (r + 1) % self.RING
        if self.events[r] is not None:
            self.events[r].synchronize()   # its upload has run (RING calls ago)
        if self.pinned[r] is None or self.pinned[r].numel() < nbytes:
            self.pinned[r] = torch.empty(nbytes + nbytes // 8, dtype=torch.uint8, pin_memory=True)
        if self.staged is None or self.staged.numel() < nbytes:
            self.staged = torch.empty(nbytes + nbytes // 8, dtype=torch.uint8, device=self.device)
        return self.pinned[r], self.staged, r


_plans: Dict[torch.device, _Plan] = {}


def _plan_for(device: torch.device) -> _Plan:
    p = _plans.get(device)
    if p is None:
        p = _plans[device] = _Plan(device)
    return p


def run_png_staged(staged: torch.Tensor, images, n: int, base: int, total: int, out: torch.Tensor,
                   device: torch.device) -> torch.Tensor:
    """The launches of a call whose staging block (describe_png_batch's layout,
    fill_png_staging's bytes) is already on its way to the device tensor `staged` (16-byte
    aligned) on the current stream.  Returns the plan's status words of the call (overwritten
    by the next call)."""
    L = _lib.lib()
    need = L.md2_png_workspace_bytes(images, n)
    if need == 0:
        _lib.check(-1, "md2_png_workspace_bytes")
    plan = _plan_for(device)
    with torch.cuda.device(device):
        plan.reserve(n, need)
        ptr = staged.data_ptr()
        _lib.check(L.md2_png_run(ptr + base, total - base, images, ptr, n, plan.workspace.data_ptr(),
                                 plan.workspace.numel(), out.data_ptr(), out.numel(), plan.status.data_ptr(),
                                 _lib.stream(device)), "md2_png_run")
    return plan.status[:n]


def run_png_staged_indexed(staged: torch.Tensor, images, index_offsets, n: int, base: int, total: int,
                           segment_bytes: int, out: torch.Tensor, device: torch.device) -> torch.Tensor:
    """run_png_staged for a block of describe_png_batch_indexed's layout (the image array, the
    index offsets behind it, then every stream with its index): md2_png_run_indexed's three
    launches on the current stream.  Returns the plan's status words of the call."""
    L = _lib.lib()
    need = L.md2_png_indexed_workspace_bytes(images, n, int(segment_bytes))
    if need == 0:
        _lib.check(-1, "md2_png_indexed_workspace_bytes")
    plan = _plan_for(device)
    with torch.cuda.device(device):
        plan.reserve(n, need)
        ptr = staged.data_ptr()
        _lib.check(L.md2_png_run_indexed(ptr + base, total - base, images, ptr, index_offsets, ptr + n * IMAGE_BYTES,
                                         n, int(segment_bytes), plan.workspace.data_ptr(), plan.workspace.numel(),
                                         out.data_ptr(), out.numel(), plan.status.data_ptr(), _lib.stream(device)),
                   "md2_png_run_indexed")
    return plan.status[:n]


def _cuda_device(device, what: str) -> torch.device:
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"{what} is GPU only (HIP kernels, no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def index_png_batch(streams: Sequence[PngStream], segment_bytes: int = SEGMENT_BYTES, device=None,
                    check: bool = True) -> List[Optional[np.ndarray]]:
    """The index of every stream for `segment_bytes` (md2_png_index: the serial walk, one
    wave per stream, no frame is written), as uint8 arrays of index_nbytes(h, w,
    segment_bytes).  Waits for the status words: a stream the inflate stage refuses raises a
    RuntimeError naming its index and bits, or with check=False gives None in its place."""
    segment_bytes = check_segment_bytes(segment_bytes)
    device = _cuda_device(device, "index_png_batch")
    n = len(streams)
    if n == 0:
        return []
    images, base, total = describe_png_batch(streams, [0] * n)
    sizes = [index_nbytes(s.height, s.width, segment_bytes) for s in streams]
    index_offsets = (ctypes.c_uint64 * n)()
    pos = 0
    for i, b in enumerate(sizes):
        index_offsets[i] = pos
        pos += b
    off_at = _align(total, 16)             # the device copy of the offsets, behind the streams
    plan = _plan_for(device)
    L = _lib.lib()
    with torch.cuda.device(device):
        pinned, staged, r = plan.stage(off_at + 8 * n)
        host = pinned.numpy()
        fill_png_staging(host, streams, images, base)
        host[off_at:off_at + 8 * n] = np.frombuffer(index_offsets, np.uint8, 8 * n)
        staged[:off_at + 8 * n].copy_(pinned[:off_at + 8 * n], non_blocking=True)
        if plan.events[r] is None:
            plan.events[r] = torch.cuda.Event()
        plan.events[r].record()
        index = torch.empty(pos, dtype=torch.uint8, device=device)
        status = torch.zeros(n, dtype=torch.int32, device=device)
        ptr = staged.data_ptr()
        _lib.check(L.md2_png_index(ptr + base, total - base, images, ptr, n, segment_bytes, index.data_ptr(), pos,
                                   index_offsets, ptr + off_at, status.data_ptr(), _lib.stream(device)),
                   "md2_png_index")
        words = status.cpu().tolist()
        flat = index.cpu().numpy()
    bad = [i for i, w in enumerate(words) if w]
    if bad and check:
        raise RuntimeError(f"index_png_batch: stream index {bad[0]} did not inflate (status {words[bad[0]]}: "
                           f"{status_text(words[bad[0]])}); bad indices {bad}")
    return [None if words[i] else flat[index_offsets[i]:index_offsets[i] + sizes[i]].copy() for i in range(n)]


def index_segment_bytes(index) -> int:
    """The segment_bytes an index was made for (its bytes 4..7)."""
    return int(np.frombuffer(bytes(index[4:8]), "<u4")[0])


def decode_png_batch_indexed(streams: Sequence[PngStream], indexes, out: torch.Tensor, offsets: Sequence[int],
                             device=None, check: bool = False, segment_bytes: Optional[int] = None) -> torch.Tensor:
    """decode_png_batch from the streams' indexes (index_png_batch's, or a pack's): the same
    contract, bytes and status words, the inflate spread over one wave per segment.  An index
    that does not fit its stream sets _lib.PNG_ST_INDEX in the stream's word; its frame is not
    written and the others are unaffected.  segment_bytes: what the indexes were made for
    (default: what the first one says)."""
    if not torch.is_tensor(out):
        raise ValueError("out must be a uint8 tensor on the device")
    device = _cuda_device(device if device is not None else out.device, "decode_png_batch_indexed")
    if out.device != device or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor on {device}")
    n = len(streams)
    if n == 0:
        return torch.zeros(0, dtype=torch.int32, device=device)
    indexes = [np.ascontiguousarray(ix, dtype=np.uint8).reshape(-1) for ix in indexes]
    if segment_bytes is None:
        segment_bytes = index_segment_bytes(indexes[0])
    segment_bytes = check_segment_bytes(segment_bytes)
    images, index_offsets, base, total = describe_png_batch_indexed(streams, indexes, offsets, segment_bytes)
    check_png_described_indexed(images, index_offsets, n, segment_bytes, total - base, out.numel())
    plan = _plan_for(device)
    with torch.cuda.device(device):
        pinned, staged, r = plan.stage(total)
        fill_png_staging_indexed(pinned.numpy(), streams, indexes, images, index_offsets, base)
        staged[:total].copy_(pinned[:total], non_blocking=True)
        if plan.events[r] is None:
            plan.events[r] = torch.cuda.Event()
        plan.events[r].record()
        status = run_png_staged_indexed(staged, images, index_offsets, n, base, total, segment_bytes, out, device)
        if check:
            bad = torch.nonzero(status.cpu()).flatten().tolist()
            if bad:
                word = int(status[bad[0]])
                raise RuntimeError(f"decode_png_batch_indexed: stream index {bad[0]} did not decode (status {word}: "
                                   f"{status_text(word)}); bad indices {bad}")
    return status


def decode_png_batch(streams: Sequence[PngStream], out: torch.Tensor, offsets: Sequence[int], device=None,
                     check: bool = False) -> torch.Tensor:
    """Decodes `streams` into the uint8 device buffer `out`: frame i is the tight (h, w, 3)
    image at byte offsets[i] (a multiple of 16); no other byte of `out` is written.  One
    asynchronous upload of one pinned block (the image array and the streams), then the two
    launches, on the current stream of `device`; nothing is allocated and nothing waits once
    the plan has grown to the batch's needs.  Returns the int32 status words of the call, one
    per stream, on the device (0 = decoded, else _lib.PNG_ST_* bits; they are the plan's and
    the next call overwrites them).  check=True synchronises and raises a RuntimeError naming
    the first index whose status is not 0."""
    device = torch.device(device) if device is not None else (out.device if torch.is_tensor(out) else None)
    if device is None or device.type != "cuda" or not torch.is_tensor(out) or not out.is_cuda:
        raise RuntimeError("decode_png_batch is GPU only (HIP kernels, no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if out.device != device or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor on {device}")
    n = len(streams)
    if n == 0:
        return torch.zeros(0, dtype=torch.int32, device=device)
    images, base, total = describe_png_batch(streams, offsets)
    check_png_described(images, n, total - base, out.numel())
    plan = _plan_for(device)
    with torch.cuda.device(device):
        pinned, staged, r = plan.stage(total)
        fill_png_staging(pinned.numpy(), streams, images, base)
        staged[:total].copy_(pinned[:total], non_blocking=True)
        if plan.events[r] is None:
            plan.events[r] = torch.cuda.Event()
        plan.events[r].record()
        status = run_png_staged(staged, images, n, base, total, out, device)
        if check:
            bad = torch.nonzero(status.cpu()).flatten().tolist()
            if bad:
                word = int(status[bad[0]])
                raise RuntimeError(f"decode_png_batch: stream index {bad[0]} did not decode (status {word}: "
                                   f"{status_text(word)}); bad indices {bad}")
    return status


def decode_png_frames(streams: Sequence[PngStream], device=None, names: Optional[Sequence[str]] = None):
    """The frames of `streams` decoded into one flat uint8 device buffer: (flat, offsets,
    sizes), frame i the tight (h, w, 3) image at byte offsets[i] (a multiple of 16) and
    sizes[i] = (h, w) — the flat form jpeg_ops.encode_jpeg_batch takes, so a frame goes from
    one codec to the other without visiting the host.  Waits for the status words and raises
    a RuntimeError naming the first stream (names[i], else its index) that did not decode."""
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("decode_png_frames is GPU only (HIP kernels, no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    offsets, sizes, pos = [], [], 0
    for s in streams:
        offsets.append(pos)
        sizes.append((s.height, s.width))
        pos += _align(s.height * s.width * 3, 16)
    with torch.cuda.device(device):
        flat = torch.empty(max(pos, 16), dtype=torch.uint8, device=device)
        status = decode_png_batch(streams, flat, offsets, device).cpu().tolist()
    bad = [i for i, w in enumerate(status) if w]
    if bad:
        who = names[bad[0]] if names is not None else f"stream index {bad[0]}"
        raise RuntimeError(f"{who} did not decode on the device (status {status[bad[0]]}: "
                           f"{status_text(status[bad[0]])}); {len(bad)} bad file(s) in its batch")
    return flat, offsets, sizes
