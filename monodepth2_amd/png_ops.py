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

The encoder (`md2_png_encode`, csrc/pngenc.hip) is the way back:
`encode_png_batch(frames)` turns device frames (8-bit RGB, 16-bit grey) into the bytes of PNG
files, filtered and deflated on the device by the rules of §6n; `png_file_bytes` wraps a zlib
stream in the chunks.  Lossless, deterministic, and not zlib's bytes.
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


# ------------------------------------------------------------------ encoding (csrc/pngenc.hip)
KIND_RGB8, KIND_GRAY16 = _lib.PNGENC_RGB8, _lib.PNGENC_GRAY16
ENC_IMAGE_BYTES = ctypes.sizeof(_lib.PngEncImage)
_BPP = {KIND_RGB8: 3, KIND_GRAY16: 2}


def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_file_bytes(height: int, width: int, kind: int, zlib_stream) -> bytes:
    """The PNG file around one zlib stream: signature, IHDR (depth 8 colour type 2 for
    KIND_RGB8, depth 16 colour type 0 for KIND_GRAY16, not interlaced), one IDAT, IEND."""
    if kind not in _BPP:
        raise ValueError(f"unknown kind {kind}")
    depth, colour = (8, 2) if kind == KIND_RGB8 else (16, 0)
    ihdr = struct.pack(">IIBBBBB", int(width), int(height), depth, colour, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", bytes(zlib_stream)) + _chunk(b"IEND", b"")


def encode_bound(height: int, width: int, kind: int, segment_bytes: int = SEGMENT_BYTES) -> int:
    """md2_png_encode_bound: a capacity no zlib stream of that geometry exceeds."""
    b = _lib.lib().md2_png_encode_bound(int(height), int(width), int(kind), int(segment_bytes))
    if b == 0:
        _lib.check(-1, "md2_png_encode_bound")
    return b


def describe_png_encode(geometries, in_offsets: Sequence[int], capacities: Optional[Sequence[int]] = None):
    """The host side of a call.  geometries: (height, width, kind, segment_bytes) per image;
    in_offsets: where each frame starts in the input bytes; capacities: the output range of
    each (default: encode_bound).  Returns (images, out_bytes, workspace_bytes): the
    md2_pngenc_image array with the output ranges laid out one after the other at 16-byte
    aligned offsets and the workspace ranges as the running sum."""
    L = _lib.lib()
    n = len(geometries)
    if n != len(in_offsets) or (capacities is not None and n != len(capacities)):
        raise ValueError(f"{n} geometries but {len(in_offsets)} offsets")
    images = (_lib.PngEncImage * max(n, 1))()
    out_pos = ws_pos = 0
    for i, (h, w, kind, s) in enumerate(geometries):
        im = images[i]
        im.height, im.width, im.kind, im.segment_bytes = int(h), int(w), int(kind), int(s)
        need = L.md2_png_encode_workspace_bytes(ctypes.byref(im), 1)
        if need == 0:
            _lib.check(-1, "md2_png_encode_workspace_bytes")
        cap = encode_bound(h, w, kind, s) if capacities is None else int(capacities[i])
        im.in_offset, im.out_offset, im.ws_offset, im.out_capacity = int(in_offsets[i]), out_pos, ws_pos, cap
        out_pos += _align(max(cap, 1), 16)
        ws_pos += need
    return images, max(out_pos, 16), ws_pos


def check_png_encode_described(images, n: int, in_bytes: int, out_bytes: int):
    """md2_png_encode's argument checks alone (host only): raises what it would refuse."""
    _lib.check(_lib.lib().md2_png_encode_check(images, n, in_bytes, out_bytes), "md2_png_encode_check")


_enc_workspaces: Dict[torch.device, torch.Tensor] = {}


def run_png_encode(flat: torch.Tensor, images, n: int, out: torch.Tensor, workspace_bytes: int,
                   device: torch.device):
    """The launches of a call on the current stream: `flat` the input bytes (uint8 view of the
    frames on the device), `images` describe_png_encode's array, `out` the uint8 output bytes.
    Returns (stream_bytes, status): uint32 words per image as int32 tensors on the device."""
    L = _lib.lib()
    with torch.cuda.device(device):
        ws = _enc_workspaces.get(device)
        if ws is None or ws.numel() < workspace_bytes:
            ws = _enc_workspaces[device] = torch.empty(workspace_bytes + workspace_bytes // 8, dtype=torch.uint8,
                                                       device=device)
        table = torch.frombuffer(bytearray(bytes(images)[:n * ENC_IMAGE_BYTES]), dtype=torch.uint8).to(device)
        words = torch.zeros(2 * n, dtype=torch.int32, device=device)
        _lib.check(L.md2_png_encode(flat.data_ptr(), flat.numel(), images, table.data_ptr(), n, ws.data_ptr(),
                                    ws.numel(), out.data_ptr(), out.numel(), words.data_ptr(),
                                    words.data_ptr() + 4 * n, _lib.stream(device)), "md2_png_encode")
    return words[:n], words[n:]


def _frame_kind(t: torch.Tensor, kind) -> int:
    if kind is None:
        if t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3:
            return KIND_RGB8
        if t.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)) and t.dim() == 2:
            return KIND_GRAY16
        raise ValueError(f"cannot tell the kind of a {t.dtype} frame of shape {tuple(t.shape)}: (h, w, 3) uint8 "
                         f"is RGB8, (h, w) int16 / uint16 is GRAY16")
    kind = int(kind)
    ok = (t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3) if kind == KIND_RGB8 else \
        (kind == KIND_GRAY16 and t.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)) and t.dim() == 2)
    if not ok:
        raise ValueError(f"a {t.dtype} frame of shape {tuple(t.shape)} is not of kind {kind}")
    return kind


def _bytes_view(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8).reshape(-1)


def encode_png_batch(frames, kind=None, segment_bytes=SEGMENT_BYTES, device=None, check: bool = False) -> List[bytes]:
    """The PNG files of device frames, filtered and deflated on the device (md2_png_encode,
    DESIGN.md §6n).  frames: a list of tensors — (h, w, 3) uint8 is 8-bit RGB, (h, w) int16 or
    uint16 (the uint16 bit patterns, as eval_ops.benchmark_depth_maps returns them) is 16-bit
    grey; sizes and kinds may be mixed — or one stacked tensor (N, h, w, 3) / (N, h, w), which
    is encoded where it lies.  kind: None (told from dtype and shape), a KIND_* or one per
    frame; segment_bytes: S, or one per frame.  One small download of the stream lengths and
    status words, then one of the compressed bytes, gathered on the device.  check=True also
    inflates every stream on the host and compares its length with the scanlines'.  GPU only."""
    stacked = torch.is_tensor(frames)
    items = list(frames.unbind(0)) if stacked else list(frames)
    if device is None and items and torch.is_tensor(items[0]) and items[0].is_cuda:
        device = items[0].device
    device = _cuda_device(device, "encode_png_batch")
    n = len(items)
    if n == 0:
        return []
    if any(not torch.is_tensor(t) or t.device != device for t in items):
        raise RuntimeError(f"encode_png_batch is GPU only (HIP kernels, no CPU fallback): every frame must be a "
                           f"tensor on {device}")
    kinds = [_frame_kind(t, k) for t, k in zip(items, kind if isinstance(kind, (list, tuple)) else [kind] * n)]
    segs = [check_segment_bytes(s) for s in
            (segment_bytes if isinstance(segment_bytes, (list, tuple)) else [segment_bytes] * n)]
    if len(segs) != n:
        raise ValueError(f"{n} frames but {len(segs)} segment sizes")
    geos = [(int(t.shape[0]), int(t.shape[1]), k, s) for t, k, s in zip(items, kinds, segs)]
    sizes = [h * w * _BPP[k] for h, w, k, _ in geos]
    with torch.cuda.device(device):
        if stacked and frames.is_contiguous():
            flat = frames.view(torch.uint8).reshape(-1)
            offsets = [i * sizes[0] for i in range(n)]
        else:
            offsets, pos = [], 0
            for b in sizes:
                offsets.append(pos)
                pos += _align(b, 16)
            flat = torch.zeros(max(pos, 16), dtype=torch.uint8, device=device)
            for t, o, b in zip(items, offsets, sizes):
                flat[o:o + b] = _bytes_view(t)
        images, out_bytes, ws_bytes = describe_png_encode(geos, offsets)
        check_png_encode_described(images, n, flat.numel(), out_bytes)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=device)
        lengths, status = run_png_encode(flat, images, n, out, ws_bytes, device)
        words = torch.cat([lengths, status]).cpu().tolist()
        lengths, status = words[:n], words[n:]
        bad = [i for i, w in enumerate(status) if w]
        if bad:
            raise RuntimeError(f"encode_png_batch: frame index {bad[0]} needs {lengths[bad[0]]} bytes, more than "
                               f"its bound {images[bad[0]].out_capacity}; bad indices {bad}")
        host = torch.cat([out[images[i].out_offset:images[i].out_offset + lengths[i]] for i in range(n)]).cpu()
        host = host.numpy().tobytes()
    files, pos = [], 0
    for (h, w, k, _), nb in zip(geos, lengths):
        z = host[pos:pos + nb]
        pos += nb
        if check and len(zlib.decompress(z)) != h * (1 + _BPP[k] * w):
            raise RuntimeError("encode_png_batch: a stream does not inflate to its scanlines")
        files.append(png_file_bytes(h, w, k, z))
    return files
