"""A packed frame file: every frame of a KITTI tree parsed, unstuffed and indexed once.

`build_pack` names the frames of some split lists through the dataset classes
(`parse(i).paths`), reads each file once, and writes one file that holds, per frame, what
the device decoder needs with no further host work: the unstuffed entropy-coded stream
(jpeg_ops.parse_jpeg), ids of its quantisation and Huffman tables, and the stream's
synchronisation index (jpeg_ops.index_jpeg_batch: the entry state of every 1024-bit
subsequence, found once on the device) directly behind it.  A file the device decoder does
not take (PNG, progressive, ...) is stored as its PIL-decoded RGB bytes, kind RAW, so a
batch from the pack is always bit-equal to the same batch from disk.  With `transcode=(quality,
sampling)` such a file is instead encoded as baseline JPEG on the device (jpeg_ops.
encode_jpeg_batch) and stored as a JPEG record under its own key: a fraction of the size and
decoded by the device decoder like the rest, but lossy; a batch from such a pack is bit-equal
to the batch from the tree after `convert_dataset` with the same quality and sampling, read
as .jpg with --device_decode.  With `png_records=True` an 8-bit RGB PNG file is instead kept
as it is, lossless and at the file's own size: a PNG record holds its deflate stream
(png_ops.parse_png) and, directly behind it, the stream's segment index
(png_ops.index_png_batch: where every segment of `segment_bytes` output bytes starts, found
once on the device), and the loader decodes it with md2_png_run_indexed; a
batch from such a pack is bit-equal to the batch from the tree.  `FramePack` opens such
a file; `loader.BatchLoader(pack=...)` then feeds the step with an index lookup and one
`os.preadv` per frame, straight into pinned memory.

The file (version 1; little-endian; every section 16-byte aligned; the header is written
last, so a build that died leaves no magic):

  header    128 bytes: magic "MD2PACK\\0", u32 version, u32 record_bytes (96), u64 file_bytes,
            u64 num_records, u32 num_quant, u32 num_huff, u64 offsets of the quant, huff,
            records and names sections, u64 names_bytes, u64 data_offset (128), zeros
  data      per record one contiguous 16-byte aligned range.  JPEG: the stream
            (stream_bytes), zeros to 16, then its index (nsub u64 states, nsub u32
            first_blocks, zeros to 16; nsub = max(ceil(8 * stream_bytes / 1024), 1)).
            RAW: height * width * 3 bytes of RGB.
            PNG: the deflate stream with its 4 trailer bytes (stream_bytes), zeros to 16,
            then its index (include/md2hot.h): u32 count, u32 segment_bytes, 8 zero bytes,
            height * (1 + 3 width) // segment_bytes + 1 entries of u64 header_bit, u64
            symbol_bit, u32 out_pos, u32 0 (the first `count` in use, the rest zero), zeros
            to 16: png_ops.index_nbytes(height, width, segment_bytes), fixed per geometry.
  quant     num_quant tables of 64 u16 in natural order   } the layout of md2_jpeg_bank:
  huff      num_huff tables of 16 counts + 256 values     } a batch's bank is a gather by id
  records   num_records x 96 bytes, sorted by name: u32 kind (0 JPEG, 1 RAW, 2 PNG), height, width,
            sampling (a PNG record: its index's segment_bytes; its table ids are zero); u64 data_offset, data_bytes; u32 stream_bytes, name_offset, name_bytes;
            u32 quant[3], dc[3], ac[3] (table ids); 16 reserved bytes: byte 0 = 1 and byte
            1 = the quality for a frame transcoded from a lossless file, else zeros (readers
            ignore them when decoding)
  names     the keys, UTF-8, back to back: a frame's path relative to --data_path with "/"

Equal tables are stored once; files written with optimised coding carry their own, so the
ids are 32-bit and the at most 255 tables of one batch are numbered per batch.
"""
from __future__ import annotations

import os
import struct
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
from PIL import Image

from . import jpeg_ops, png_ops
from ._lib import JPEG_HUFF_BYTES, JPEG_QUANT_BYTES

MAGIC = b"MD2PACK\0"
VERSION = 1
HEADER_BYTES = 128
KIND_JPEG, KIND_RAW, KIND_PNG = 0, 1, 2
_HEADER = struct.Struct("<8sIIQQIIQQQQQQ")
RECORD = np.dtype([("kind", "<u4"), ("height", "<u4"), ("width", "<u4"), ("sampling", "<u4"),
                   ("data_offset", "<u8"), ("data_bytes", "<u8"),
                   ("stream_bytes", "<u4"), ("name_offset", "<u4"), ("name_bytes", "<u4"),
                   ("quant", "<u4", 3), ("dc", "<u4", 3), ("ac", "<u4", 3), ("reserved", "u1", 16)])
assert RECORD.itemsize == 96 and _HEADER.size <= HEADER_BYTES


class PackError(ValueError):
    """A file that is no frame pack of this version, or a damaged one."""


def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


def frame_key(path: str, data_path: str) -> str:
    """A frame's key in a pack: its path relative to the dataset root, with "/"."""
    root = os.path.join(data_path, "")
    rel = path[len(root):] if path.startswith(root) else os.path.relpath(path, data_path)
    return rel.replace(os.sep, "/")


class PackRecord:
    """One frame on its way into a pack.  JPEG: `stream` (a jpeg_ops.JpegStream) and `index`
    (its index bytes, jpeg_ops.index_jpeg_batch's or pack_index's).  PNG: `stream` (a
    png_ops.PngStream) and `index` (png_ops.index_png_batch's; its segment_bytes is read
    from it).  RAW: `raw`, the decoded
    (h, w, 3) uint8 RGB frame.  `transcoded`: the quality a lossless file was encoded with on
    its way in (0: the stream is the file's own)."""
    __slots__ = ("name", "stream", "index", "raw", "transcoded")

    def __init__(self, name: str, stream=None, index=None, raw=None, transcoded: int = 0):
        if (stream is None) == (raw is None):
            raise ValueError(f"{name}: a record is either a stream with its index or raw RGB")
        if isinstance(stream, png_ops.PngStream):
            index = np.ascontiguousarray(index, dtype=np.uint8).reshape(-1)
            if index.size < 16:
                raise ValueError(f"{name}: an index of {index.size} bytes: a PNG index starts with 16 header bytes")
            want = png_ops.index_nbytes(stream.height, stream.width, png_ops.index_segment_bytes(index))
            if index.size != want:
                raise ValueError(f"{name}: an index of {index.size} bytes for a {stream.height} x {stream.width} "
                                 f"frame (expected {want} at segment_bytes {png_ops.index_segment_bytes(index)})")
        elif stream is not None:
            index = np.ascontiguousarray(index, dtype=np.uint8).reshape(-1)
            if index.size != jpeg_ops.index_nbytes(len(stream.data)):
                raise ValueError(f"{name}: an index of {index.size} bytes for a stream of {len(stream.data)} bytes "
                                 f"(expected {jpeg_ops.index_nbytes(len(stream.data))})")
        else:
            raw = np.ascontiguousarray(raw, dtype=np.uint8)
            if raw.ndim != 3 or raw.shape[2] != 3:
                raise ValueError(f"{name}: raw frames are (h, w, 3) uint8, not {raw.shape}")
        if transcoded and (stream is None or isinstance(stream, png_ops.PngStream)
                           or not 1 <= int(transcoded) <= 100):
            raise ValueError(f"{name}: a transcoded record is a stream with its quality, 1..100")
        self.name, self.stream, self.index, self.raw, self.transcoded = name, stream, index, raw, int(transcoded)


def _huff_bytes(counts, vals) -> bytes:
    return bytes(counts) + bytes(vals) + b"\0" * (JPEG_HUFF_BYTES - 16 - len(vals))


def write_pack(path: str, records: Iterable[PackRecord]) -> int:
    """Writes the records (any order, any iterable: data is written as it arrives) to `path`;
    returns their number.  Records already carry their index.  Two records of one name are
    refused."""
    quant: Dict[bytes, int] = {}
    huff: Dict[bytes, int] = {}
    rows: List[Tuple] = []
    seen = set()
    with open(path, "wb") as f:
        f.write(b"\0" * HEADER_BYTES)
        pos = HEADER_BYTES
        for rec in records:
            if rec.name in seen:
                raise ValueError(f"{rec.name}: twice in one pack")
            seen.add(rec.name)
            if isinstance(rec.stream, png_ops.PngStream):
                s = rec.stream
                pad = _align16(len(s.data)) - len(s.data)
                f.write(s.data)
                f.write(b"\0" * pad)
                f.write(rec.index.tobytes())
                nbytes = len(s.data) + pad + rec.index.size
                rows.append((rec.name, KIND_PNG, s.height, s.width, png_ops.index_segment_bytes(rec.index), pos, nbytes,
                             len(s.data), [0] * 3, [0] * 3, [0] * 3, 0))
            elif rec.stream is not None:
                s = rec.stream
                pad = _align16(len(s.data)) - len(s.data)
                f.write(s.data)
                f.write(b"\0" * pad)
                f.write(rec.index.tobytes())
                nbytes = len(s.data) + pad + rec.index.size
                q = [quant.setdefault(np.asarray(s.quant[c], dtype="<u2").tobytes(), len(quant)) for c in range(3)]
                dc = [huff.setdefault(_huff_bytes(*s.huff[(0, s.dc[c])]), len(huff)) for c in range(3)]
                ac = [huff.setdefault(_huff_bytes(*s.huff[(1, s.ac[c])]), len(huff)) for c in range(3)]
                rows.append((rec.name, KIND_JPEG, s.height, s.width, s.sampling, pos, nbytes, len(s.data), q, dc, ac,
                             rec.transcoded))
            else:
                h, w = rec.raw.shape[:2]
                f.write(rec.raw.tobytes())
                nbytes = _align16(h * w * 3)
                f.write(b"\0" * (nbytes - h * w * 3))
                rows.append((rec.name, KIND_RAW, h, w, 0, pos, h * w * 3, 0, [0] * 3, [0] * 3, [0] * 3, 0))
            pos += nbytes
        rows.sort(key=lambda r: r[0])
        table = np.zeros(len(rows), RECORD)
        names = bytearray()
        for i, (name, kind, h, w, sampling, off, nbytes, sbytes, q, dc, ac, transcoded) in enumerate(rows):
            key = name.encode("utf-8")
            reserved = np.zeros(16, np.uint8)
            if transcoded:
                reserved[0], reserved[1] = 1, transcoded
            table[i] = (kind, h, w, sampling, off, nbytes, sbytes, len(names), len(key), q, dc, ac, reserved)
            names += key
        quant_off = pos
        f.write(b"".join(quant))                      # dicts keep insertion order: id order
        huff_off = quant_off + _align16(len(quant) * JPEG_QUANT_BYTES)
        f.seek(huff_off)
        f.write(b"".join(huff))
        rec_off = huff_off + _align16(len(huff) * JPEG_HUFF_BYTES)
        f.seek(rec_off)
        f.write(table.tobytes())
        names_off = rec_off + _align16(table.nbytes)
        f.seek(names_off)
        f.write(bytes(names))
        total = _align16(names_off + len(names))
        f.truncate(total)
        f.seek(0)
        f.write(_HEADER.pack(MAGIC, VERSION, RECORD.itemsize, total, len(rows), len(quant), len(huff), quant_off,
                             huff_off, rec_off, names_off, len(names), HEADER_BYTES))
    return len(rows)


class FramePack:
    """A pack opened for reading: the header validated, the tables, records and names in
    memory, the data left on disk behind one file descriptor (`read_into`, thread-safe)."""

    def __init__(self, path: str):
        self.path = str(path)
        self._fd = None
        size = os.path.getsize(self.path)
        with open(self.path, "rb") as f:
            head = f.read(HEADER_BYTES)
            if len(head) < HEADER_BYTES:
                raise PackError(f"{self.path}: truncated: {len(head)} bytes, a pack header has {HEADER_BYTES}")
            (magic, version, rbytes, total, n, nq, nh, q_off, h_off, r_off, n_off, n_bytes,
             d_off) = _HEADER.unpack_from(head)
            if magic != MAGIC:
                raise PackError(f"{self.path}: wrong magic {magic!r}: not a frame pack (or one whose build did not "
                                "finish)")
            if version != VERSION or rbytes != RECORD.itemsize:
                raise PackError(f"{self.path}: wrong version {version} (records of {rbytes} bytes): this build reads "
                                f"version {VERSION} (records of {RECORD.itemsize} bytes)")
            if size < total:
                raise PackError(f"{self.path}: truncated: {size} bytes on disk, the header says {total}")
            ends = [(q_off, nq * JPEG_QUANT_BYTES), (h_off, nh * JPEG_HUFF_BYTES), (r_off, n * rbytes),
                    (n_off, n_bytes)]
            if d_off != HEADER_BYTES or any(o % 16 or o < d_off or o + b > total for o, b in ends):
                raise PackError(f"{self.path}: a section lies outside the file's {total} bytes")

            def section(off, nbytes):
                f.seek(off)
                b = f.read(nbytes)
                if len(b) != nbytes:
                    raise PackError(f"{self.path}: truncated inside a section")
                return b

            self.quant = np.frombuffer(section(q_off, nq * JPEG_QUANT_BYTES), np.uint8).reshape(nq, JPEG_QUANT_BYTES)
            self.huff = np.frombuffer(section(h_off, nh * JPEG_HUFF_BYTES), np.uint8).reshape(nh, JPEG_HUFF_BYTES)
            self.records = np.frombuffer(section(r_off, n * rbytes), RECORD)
            names = section(n_off, n_bytes)
        self.file_bytes = total
        r = self.records
        if n:
            jpeg = r["kind"] == KIND_JPEG
            if (np.any(r["data_offset"] % 16) or np.any(r["data_offset"] < d_off)
                    or np.any(r["data_offset"] + r["data_bytes"] > q_off) or np.any(r["kind"] > KIND_PNG)
                    or np.any(r["name_offset"].astype(np.uint64) + r["name_bytes"] > n_bytes)
                    or np.any(r["quant"][jpeg] >= nq) or np.any(r["dc"][jpeg] >= nh) or np.any(r["ac"][jpeg] >= nh)):
                raise PackError(f"{self.path}: a record points outside its section")
        # PNG records: one segment_bytes for the whole pack (a batch is one call), and every
        # record as long as its stream and its geometry's index say
        self.png_segment_bytes = 0
        png = np.flatnonzero(r["kind"] == KIND_PNG) if n else []
        if len(png):
            sb = {int(x) for x in r["sampling"][png]}
            try:
                if len(sb) != 1:
                    raise ValueError(f"PNG records with different segment_bytes {sorted(sb)}")
                self.png_segment_bytes = png_ops.check_segment_bytes(sb.pop())
                h, w = r["height"][png].astype(np.int64), r["width"][png].astype(np.int64)
                if np.any(h < 1) or np.any(h > png_ops.MAX_DIM) or np.any(w < 1) or np.any(w > png_ops.MAX_DIM):
                    raise ValueError(f"a PNG record's height or width is outside 1..{png_ops.MAX_DIM}")
                sbytes = r["stream_bytes"][png].astype(np.int64)
                entries = h * (1 + 3 * w) // self.png_segment_bytes + 1          # png_ops.index_nbytes, for all rows
                want = (sbytes + 15) // 16 * 16 + (16 + 24 * entries + 15) // 16 * 16
                wrong = np.flatnonzero((r["data_bytes"][png].astype(np.int64) != want) | (sbytes < 5))
                if len(wrong):
                    i = int(png[wrong[0]])
                    raise ValueError(f"PNG record {i}: {int(r['data_bytes'][i])} data bytes, but its stream of "
                                     f"{int(r['stream_bytes'][i])} bytes and the index of a {int(r['height'][i])} x "
                                     f"{int(r['width'][i])} frame take {int(want[wrong[0]])}")
            except ValueError as e:
                raise PackError(f"{self.path}: {e}") from None
        self.names = [names[int(o):int(o) + int(b)].decode("utf-8") for o, b in zip(r["name_offset"], r["name_bytes"])]
        self._row = {name: i for i, name in enumerate(self.names)}
        # what the loader asks per frame, as plain Python values
        self._sizes = [(int(h), int(w)) for h, w in zip(r["height"], r["width"])]
        # frames encoded from lossless files when the pack was built (build_pack's transcode)
        self.transcoded = int(np.count_nonzero(r["reserved"][:, 0] == 1)) if n else 0
        self._fd = os.open(self.path, os.O_RDONLY)

    def __len__(self):
        return len(self.names)

    def __contains__(self, key: str):
        return key in self._row

    def row(self, key: str) -> int:
        try:
            return self._row[key]
        except KeyError:
            raise KeyError(f"{key} is not in the pack {self.path}") from None

    def record(self, key: str):
        """The record (a numpy row of dtype RECORD) of the frame with key `key`."""
        return self.records[self.row(key)]

    def size(self, key: str) -> Tuple[int, int]:
        """(height, width) of the frame with key `key`."""
        return self._sizes[self.row(key)]

    def read_into(self, row: int, dest: np.ndarray):
        """Record `row`'s byte range read into `dest` (uint8, data_bytes long): one preadv."""
        rec = self.records[row]
        want = int(rec["data_bytes"])
        got = os.preadv(self._fd, [memoryview(dest)], int(rec["data_offset"]))
        while 0 < got < want:       # a short read continues where it stopped
            more = os.preadv(self._fd, [memoryview(dest)[got:]], int(rec["data_offset"]) + got)
            if more <= 0:
                break
            got += more
        if got != want:
            raise IOError(f"{self.path}: {got} of {want} bytes read for {self.names[row]}")

    def read(self, key: str) -> np.ndarray:
        """The frame's bytes: stream, padding and index of a JPEG record, RGB of a RAW one."""
        row = self.row(key)
        out = np.empty(int(self.records[row]["data_bytes"]), np.uint8)
        self.read_into(row, out)
        return out

    def stream(self, key: str):
        """(JpegStream, index bytes) of a JPEG record, as write_pack took them."""
        rec = self.record(key)
        if rec["kind"] != KIND_JPEG:
            raise ValueError(f"{key} is a {'PNG' if rec['kind'] == KIND_PNG else 'RAW'} record")
        data = self.read(key)
        n = int(rec["stream_bytes"])
        huff, dc, ac = {}, [], []
        for c in range(3):
            for cls, ids, out in ((0, rec["dc"], dc), (1, rec["ac"], ac)):
                t = self.huff[int(ids[c])]
                counts = tuple(int(x) for x in t[:16])
                huff[(cls, int(ids[c]))] = (counts, t[16:16 + sum(counts)].tobytes())
                out.append(int(ids[c]))
        quant = tuple(tuple(int(x) for x in self.quant[int(rec["quant"][c])].view("<u2")) for c in range(3))
        factors = {v: k for k, v in jpeg_ops.SAMPLINGS.items()}[int(rec["sampling"])]
        s = jpeg_ops.JpegStream(int(rec["height"]), int(rec["width"]), int(rec["sampling"]), factors, quant, huff,
                                tuple(dc), tuple(ac), data[:n].tobytes())
        return s, data[_align16(n):].copy()

    def png_stream(self, key: str):
        """(PngStream, index bytes) of a PNG record, as write_pack took them."""
        rec = self.record(key)
        if rec["kind"] != KIND_PNG:
            raise ValueError(f"{key} is a {'JPEG' if rec['kind'] == KIND_JPEG else 'RAW'} record")
        data = self.read(key)
        n = int(rec["stream_bytes"])
        return png_ops.PngStream(int(rec["height"]), int(rec["width"]), data[:n].tobytes()), data[_align16(n):].copy()

    def missing(self, dataset) -> Optional[str]:
        """None if the pack holds every frame of every split line of `dataset`, else a
        sentence naming the first line and path it lacks."""
        for i in range(len(dataset)):
            item = dataset.parse(i)
            for p in item.paths:
                if frame_key(p, dataset.data_path) not in self._row:
                    return (f"split line {i} ({item.line!r}): {p} is not in the pack {self.path} "
                            f"(key {frame_key(p, dataset.data_path)!r}; {len(self)} frames packed)")
        return None

    def covers(self, dataset) -> bool:
        """Whether the pack holds every frame of every split line of `dataset` (`missing` says which not)."""
        return self.missing(dataset) is None

    def close(self):
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def open_pack(opt) -> Optional[FramePack]:
    """The pack --pack names, or None without the flag."""
    path = getattr(opt, "pack", None)
    if not path:
        return None
    pack = FramePack(path)
    if pack.transcoded:
        qualities = sorted({int(q) for q in pack.records["reserved"][pack.records["reserved"][:, 0] == 1, 1]})
        print(f"{path}: {pack.transcoded} of {len(pack)} frames are lossy JPEG transcodes of PNG files (quality "
              f"{', '.join(map(str, qualities))}): they decode as the tree would after convert_dataset, not as the PNGs")
    return pack


def frame_paths(data_path: str, line_lists: Sequence[Sequence[str]], dataset: str = "kitti", png: bool = False,
                frame_ids: Sequence = (0, -1, 1), use_stereo: bool = False) -> Dict[str, str]:
    """{key: path} of every frame the split lines name, through the dataset class's own
    `parse(i).paths`, deduplicated."""
    from .datasets import DATASETS
    if dataset not in DATASETS:
        raise ValueError(f"--dataset {dataset} cannot be packed: choose one of {sorted(DATASETS)}")
    ids = list(frame_ids) + (["s"] if use_stereo and "s" not in frame_ids else [])
    out: Dict[str, str] = {}
    for lines in line_lists:
        ds = DATASETS[dataset](data_path, list(lines), 192, 640, ids, 4, is_train=False,
                               img_ext=".png" if png else ".jpg")
        for i in range(len(ds)):
            for p in ds.parse(i).paths:
                out.setdefault(frame_key(p, data_path), p)
    return out


def records_from_files(paths: Dict[str, str], device=None, batch: int = 64, threads: int = 8,
                       transcode: Optional[Tuple[int, object]] = None,
                       device_png: bool = False, png_records: bool = False,
                       segment_bytes: int = png_ops.SEGMENT_BYTES) -> Iterator[PackRecord]:
    """The records of the files {key: path}, in key order: read and parsed by `threads` host
    threads, the supported JPEG files indexed on the device `batch` at a time, every other
    file decoded with PIL into a RAW record.  transcode=(quality, sampling): such a file is
    encoded on the device after PIL decoded it, indexed with the rest of its batch and
    becomes a JPEG record under its own key, marked as transcoded.  With device_png as well,
    the PNG files png_ops.parse_png takes are not decoded by PIL: the device decodes them into
    a flat buffer that goes straight into the encoder (the same records, byte for byte).  RAW
    records keep the PIL route: their frames have to be on the host anyway.
    png_records (not with transcode): a PNG file png_ops.parse_png takes becomes a PNG record,
    its stream indexed on the device for segment_bytes with the rest of its batch and decoded
    from that index once as a check; a file the parser, the indexer or that decode refuses
    stays a RAW record through PIL."""
    if png_records and transcode is not None:
        raise ValueError("png_records and transcode exclude each other: a PNG file is either kept lossless as a "
                         "PNG record or encoded as JPEG")
    on_device_png = (bool(device_png) and transcode is not None) or bool(png_records)

    def load(key):
        path = paths[key]
        try:
            with open(path, "rb") as f:
                data = f.read()
        except FileNotFoundError:
            raise FileNotFoundError(f"no such image file {path} (frame {key})") from None
        s = jpeg_ops.parse_jpeg(data)
        if s is None and on_device_png:
            s = png_ops.parse_png(data)
        if s is not None:
            return s
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))

    keys = sorted(paths)
    with ThreadPoolExecutor(max(threads, 1)) as pool:
        for start in range(0, len(keys), batch):
            chunk = keys[start:start + batch]
            got = list(pool.map(load, chunk))
            encoded, png_kept = {}, {}
            if transcode is not None:
                pngs = [n for n, g in enumerate(got) if isinstance(g, png_ops.PngStream)]
                if pngs:
                    flat, offsets, sizes = png_ops.decode_png_frames([got[n] for n in pngs], device,
                                                                     names=[paths[chunk[n]] for n in pngs])
                    streams = jpeg_ops.encode_jpeg_batch(flat, quality=transcode[0], sampling=transcode[1],
                                                         device=device, check=True, offsets=offsets, sizes=sizes)
                    for n, s in zip(pngs, streams):
                        got[n] = s
                        encoded[n] = int(transcode[0])
                lossless = [n for n, g in enumerate(got) if not isinstance(g, jpeg_ops.JpegStream)]
                streams = jpeg_ops.encode_jpeg_batch([got[n] for n in lossless], quality=transcode[0],
                                                     sampling=transcode[1], device=device, check=True)
                for n, s in zip(lossless, streams):
                    got[n] = s
                    encoded[n] = int(transcode[0])
            if png_records:
                pngs = [n for n, g in enumerate(got) if isinstance(g, png_ops.PngStream)]
                png_indexes = _checked_png_indexes([got[n] for n in pngs], segment_bytes, device) if pngs else []
                for n, ix in zip(pngs, png_indexes):
                    if ix is None:   # refused on the device: PIL's frame, as without the flag
                        with Image.open(paths[chunk[n]]) as im:
                            got[n] = np.asarray(im.convert("RGB"))
                    else:
                        png_kept[n] = ix
            on_device = [n for n, g in enumerate(got) if isinstance(g, jpeg_ops.JpegStream)]
            indexes = dict(zip(on_device, jpeg_ops.index_jpeg_batch([got[n] for n in on_device], device)))
            for n, key in enumerate(chunk):
                if n in png_kept:
                    yield PackRecord(key, stream=got[n], index=png_kept[n])
                elif n in indexes:
                    yield PackRecord(key, stream=got[n], index=indexes[n], transcoded=encoded.get(n, 0))
                else:
                    yield PackRecord(key, raw=got[n])


def _checked_png_indexes(streams, segment_bytes: int, device) -> List[Optional[np.ndarray]]:
    """index_png_batch's indexes, with None for a stream the indexer refuses or whose decode
    from its index reports a bit (a wrong Adler-32, a bad filter byte)."""
    import torch
    indexes = png_ops.index_png_batch(streams, segment_bytes, device, check=False)
    good = [i for i, ix in enumerate(indexes) if ix is not None]
    if good:
        offsets, pos = [], 0
        for i in good:
            offsets.append(pos)
            pos += _align16(streams[i].height * streams[i].width * 3)
        dev = torch.device(device) if device is not None else torch.device("cuda")
        out = torch.empty(max(pos, 16), dtype=torch.uint8, device=dev)
        words = png_ops.decode_png_batch_indexed([streams[i] for i in good], [indexes[i] for i in good], out, offsets,
                                                 dev, segment_bytes=segment_bytes).cpu().tolist()
        for i, w in zip(good, words):
            if w:
                indexes[i] = None
    return indexes


def build_pack(out: str, data_path: str, line_lists: Sequence[Sequence[str]], dataset: str = "kitti",
               png: bool = False, frame_ids: Sequence = (0, -1, 1), use_stereo: bool = False, device=None,
               batch: int = 64, threads: int = 8, transcode: Optional[Tuple[int, object]] = None,
               device_png: bool = False, png_records: bool = False,
               segment_bytes: int = png_ops.SEGMENT_BYTES) -> Dict:
    """Parse, index on the device, write: the frames the split lines of `line_lists` name
    under `data_path`, into the pack `out`.  Files are read by `threads` host threads and
    indexed `batch` at a time.  transcode=(quality, sampling): files the device decoder does
    not take are encoded as JPEG on the device instead of stored decoded (records_from_files);
    device_png: the PNG files among them are decoded on the device too.  png_records (not
    with transcode): 8-bit RGB PNG files are kept lossless as PNG records with a segment index
    for segment_bytes.
    Returns {"frames", "jpeg", "raw", "png", "transcoded", "pack_bytes", "file_bytes"}
    (file_bytes: the size of the image files read; transcoded frames count as jpeg too)."""
    if png_records and transcode is not None:
        raise ValueError("png_records and transcode exclude each other: a PNG file is either kept lossless as a "
                         "PNG record or encoded as JPEG")
    if png_records:
        png_ops.check_segment_bytes(segment_bytes)
    paths = frame_paths(data_path, line_lists, dataset, png, frame_ids, use_stereo)
    stats = {"frames": 0, "jpeg": 0, "raw": 0, "png": 0, "transcoded": 0, "file_bytes": 0}
    if transcode is not None:
        transcode = (int(transcode[0]), jpeg_ops.sampling_class(transcode[1]))
        jpeg_ops.quality_tables(transcode[0])

    def counted():
        for rec in records_from_files(paths, device, batch, threads, transcode, device_png, png_records,
                                      segment_bytes):
            stats["png" if isinstance(rec.stream, png_ops.PngStream) else
                  "jpeg" if rec.stream is not None else "raw"] += 1
            stats["transcoded"] += 1 if rec.transcoded else 0
            stats["file_bytes"] += os.path.getsize(paths[rec.name])
            yield rec

    tmp = out + ".tmp"
    try:
        stats["frames"] = write_pack(tmp, counted())
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    stats["pack_bytes"] = os.path.getsize(out)
    return stats
