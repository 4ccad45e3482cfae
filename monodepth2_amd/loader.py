"""Batch loader: split lines -> decoded frames in pinned memory -> one upload -> the GPU
input pipeline -> the dict `Trainer.train_step` / `val_step` take.

Stands where the reference has `DataLoader(dataset, batch_size, shuffle, num_workers,
pin_memory=True, drop_last=True)` (trainer.py:127-139) around a dataset whose
`__getitem__` did all the PIL work.  Here the dataset only names and decodes files
(datasets.py) and the per-item work runs on the GPU for the whole batch
(augment.GpuAugmentMixed), so a batch is:

  1. the epoch's permutation (drawn from `seed` and the epoch), cut into batches with the
     last partial one dropped, batches dealt to ranks as `rank::world_size` (with
     `drop_last=False`, the evaluators' order, the partial batch is produced too: one
     process only, and a second GPU plan of the tail's size, since a plan's batch is fixed);
  2. every image file of the batch opened (sizes are known from the headers), frame
     offsets laid out 256-byte aligned in one ragged buffer;
  3. the frames decoded by up to min(num_workers, 16) THREADS (PIL releases the GIL while
     it decodes; no process is forked or spawned beside one that has the GPU open) and
     copied into one of a small ring of pinned buffers;
  4. one asynchronous host-to-device copy of that buffer and one `GpuAugmentMixed` call.

Steps 2-3 of the next `prefetch` batches run on a producer thread while the caller trains
on the current one.  That thread and the decoding threads do host work only: every call
into the HIP runtime (allocating the pinned ring, uploads, events and waiting for them) is
made on the caller's thread, between its steps, so none can fall into a graph capture the
caller has open on another stream (a host allocation from a second thread is refused
while a global-mode capture runs).  The ring is allocated when an epoch starts, sized from
its first batch with an eighth to spare; a later batch that needs more is decoded into
pageable memory and its slot grown on the caller's thread.  A pinned buffer goes back to
the producer only after the event recorded behind its upload has completed, two batches
later; nothing here calls torch.cuda.synchronize().

`device_decode=True` moves the JPEG decoder onto the device (jpeg_ops, csrc/jpeg.hip): the
decoding threads read each file and parse its headers; a supported baseline JPEG goes up
as its unstuffed entropy-coded segment (about a seventh of its pixels) and is decoded by
the kernels straight into the ragged buffer, anything else (PNG, progressive, ...) is
decoded with PIL as before, uploaded in the same block and moved to its place by a device
copy.  Every rule above stands.  The decoder's status words come back through pinned memory
behind the slot's event and are read when the slot is retired: a stream that did not decode
raises a RuntimeError naming the split line and the file, one or two batches after its own
or when the epoch ends.

`device_png=True` (implies device_decode) sends 8-bit RGB PNG files the same
way: a file `jpeg_ops.parse_jpeg` refuses is offered to `png_ops.parse_png`, the deflate
streams get a region of their own in the staging block behind the JPEG one, `md2_png_run`
inflates and unfilters them into the ragged buffer, and their status words follow the JPEG
streams' through the same pinned copy.  Gray, palette, alpha, 16-bit and interlaced files stay
with PIL (`pil_fallbacks` counts the frames PIL decoded).  A pack's PNG records need no flag:
they carry a segment index and go through `md2_png_run_indexed`.

`pack=FramePack(...)` (pack.py) feeds the same device decoder from a packed
frame file instead of the image files: sizes come from the pack's records and no file is
opened; the producer thread lays the staging block out (the batch's table bank gathered from
the records' ids, then every frame's record) and the decoding threads `os.preadv` each
record, the stream with its synchronisation index behind it, straight into the slot's pinned
buffer; the caller's thread launches `md2_jpeg_run_indexed`.  RAW records (files the device
decoder does not take, stored decoded) ride the PIL frames' route.  Implies device_decode.
"""
from __future__ import annotations

import collections
import ctypes
import queue
import random
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterator, List, Optional

import numpy as np
import torch

from . import _lib, jpeg_ops, png_ops
from .augment import GpuAugmentMixed
from .datasets import item_seed
from .pack import KIND_JPEG, KIND_PNG, frame_key

ALIGN = 256        # frame offsets in the ragged buffer
MAX_THREADS = 16   # decoding threads, whatever --num_workers asks for
IN_FLIGHT = 2      # uploads that may still be running when a batch is handed out


def _padded(size) -> int:
    return (size[0] * size[1] * 3 + ALIGN - 1) // ALIGN * ALIGN


class _Staged:
    """A batch decoded into ring slot `slot`, ready for its upload.  `spill`: the frames
    in pageable memory, where the slot's pinned buffer was too small for them."""

    def __init__(self, slot, total, offsets, items, spill=None):
        self.slot, self.total, self.offsets, self.items, self.spill = slot, total, offsets, items, spill
        self.jpeg = None   # device_decode: a _StagedJpeg; `total` then counts the staging block, not the frames


class _StagedJpeg:
    """What a device-decoded batch adds: the decoder's host description, the frames PIL
    decoded instead as (frame number, offset in the staging block, bytes), the size of the
    ragged frame buffer and, per stream, the split line and file to name in an error."""

    def __init__(self, images, n, num_quant, num_huff, base, jtotal, pil, frames_total, names):
        self.images, self.n, self.num_quant, self.num_huff = images, n, num_quant, num_huff
        self.base, self.jtotal = base, jtotal
        self.pil, self.frames_total, self.names = pil, frames_total, names
        self.index_offsets = None   # a packed batch: where each stream's index lies, for md2_jpeg_run_indexed
        self.png = None             # device_png: a _StagedPng, the PNG streams' own region of the block


class _StagedPng:
    """The PNG streams of a device-decoded batch: png_ops.describe_png_batch's description and
    where its region starts in the staging block."""

    def __init__(self, images, n, offset, base, total):
        self.images, self.n, self.offset, self.base, self.total = images, n, offset, base, total
        self.index_offsets = None   # a packed batch: where each stream's index lies, for md2_png_run_indexed
        self.segment_bytes = 0      # ... and the segment_bytes of the pack's indexes


class BatchLoader:
    def __init__(self, dataset, batch_size: int, shuffle: bool = True, seed: int = 0, num_workers: int = 0,
                 rank: int = 0, world_size: int = 1, device=None, with_depth: bool = False, prefetch: int = 2,
                 drop_last: bool = True, device_decode: bool = False, pack=None, device_png: bool = False):
        if not (0 <= rank < world_size):
            raise ValueError(f"rank {rank} outside world size {world_size}")
        if not drop_last and world_size > 1:
            raise ValueError("drop_last=False is the evaluation order, one process: it cannot be dealt to "
                             f"world_size {world_size} ranks in equal steps")
        self.drop_last = bool(drop_last)
        self.dataset = dataset
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.seed = seed
        self.threads = min(max(int(num_workers), 0), MAX_THREADS)
        self.rank, self.world_size = rank, world_size
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("BatchLoader feeds the GPU input pipeline (no CPU fallback)")
        if with_depth and not getattr(dataset, "load_depth", False):
            raise ValueError("with_depth needs a dataset built with load_depth=True whose first split line has "
                             "ground truth (check_depth)")
        self.with_depth = with_depth
        self.device_png = bool(device_png) and pack is None   # a pack holds no PNG streams
        self.device_decode = bool(device_decode) or self.device_png or pack is not None
        self.pil_fallbacks = 0    # device_decode: frames PIL decoded because no device decoder takes their file
        self.pack = pack
        if pack is not None:   # every frame of every split line, before anything is built
            lacking = pack.missing(dataset)
            if lacking:
                raise ValueError(lacking)
        self.prefetch = max(int(prefetch), 1)
        self.epoch = 0
        self.uploaded_bytes = 0   # host-to-device bytes of the batches handed out so far (tools/loader_bench.py)
        self.frame_ids = list(dataset.frame_idxs)
        self.aug = GpuAugmentMixed(dataset.height, dataset.width, self.frame_ids, batch_size, dataset.num_scales,
                                   device=self.device)
        self._tail_aug: Optional[GpuAugmentMixed] = None   # drop_last=False: the partial batch's plan
        # ring: one slot being filled, `prefetch` queued, IN_FLIGHT whose upload may be running
        self._ring = self.prefetch + 1 + IN_FLIGHT
        self._pinned: List[Optional[torch.Tensor]] = [None] * self._ring
        self._uploaded: List[Optional[torch.cuda.Event]] = [None] * self._ring
        # device_decode: per slot the decoder's status words (pinned) and whom they belong to
        self._status: List[Optional[torch.Tensor]] = [None] * self._ring
        self._status_of: List[Optional[List]] = [None] * self._ring
        self._pool = ThreadPoolExecutor(self.threads, thread_name_prefix="md2-decode") if self.threads else None

    # ------------------------------------------------------------------ order
    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def batches(self, epoch: Optional[int] = None) -> List[List[int]]:
        """This rank's batches of dataset indices for `epoch`."""
        epoch = self.epoch if epoch is None else epoch
        order = list(range(len(self.dataset)))
        if self.shuffle:
            random.Random(item_seed(self.seed, epoch, -1)).shuffle(order)
        B = self.batch_size
        full = [order[i * B:(i + 1) * B] for i in range(len(order) // B)]   # drop_last
        if not self.drop_last:                                              # one rank: every item, the tail too
            return full + ([order[len(full) * B:]] if len(order) % B else [])
        per_rank = len(full) // self.world_size                             # equal steps on every rank
        return full[self.rank::self.world_size][:per_rank]

    def __len__(self):
        if not self.drop_last:
            return -(-len(self.dataset) // self.batch_size)
        return (len(self.dataset) // self.batch_size) // self.world_size

    def _aug_for(self, n: int) -> GpuAugmentMixed:
        """The plan of a batch of `n` items: a plan's batch size is fixed, so the partial
        last batch of drop_last=False gets one of its own, built when it is first met."""
        if n == self.batch_size:
            return self.aug
        if self._tail_aug is None or self._tail_aug.batch_size != n:
            self._tail_aug = GpuAugmentMixed(self.dataset.height, self.dataset.width, self.frame_ids, n,
                                             self.dataset.num_scales, device=self.device)
        return self._tail_aug

    # ---------------------------------------------------------------- staging
    def _map(self, fn, seq):
        return list(self._pool.map(fn, seq)) if self._pool is not None else [fn(x) for x in seq]

    def _open(self, indices: List[int], epoch: int):
        """Step 2: the batch's items with their image files open.  If one item fails, the
        files of the others are closed before its error is raised."""
        def one(i):
            try:
                return self.dataset.open_item(i, epoch)
            except BaseException as e:
                return e

        items = self._map(one, indices)
        errors = [it for it in items if isinstance(it, BaseException)]
        if errors:
            for it in items:
                if not isinstance(it, BaseException):
                    it.close()
            raise errors[0]
        return items

    def _open_packed(self, indices: List[int], epoch: int):
        """Step 2 from a pack: the items with their sizes from the records; no file is opened.
        Every item carries its frames' record rows in `rows`."""
        items = []
        for i in indices:
            it = self.dataset.parse(i, epoch)
            it.rows = [self.pack.row(frame_key(p, self.dataset.data_path)) for p in it.paths]
            sizes = {self.pack._sizes[r] for r in it.rows}
            if len(sizes) != 1:
                raise ValueError(f"split line {i} ({it.line!r}): its frames decode to different sizes "
                                 f"{sorted(sizes)}: {it.paths}")
            it.size = sizes.pop()
            items.append(it)
        return items

    def _stage(self, indices: List[int], epoch: int, slot: int) -> _Staged:
        """Steps 2-3 for one batch into the free ring slot `slot`: host work only."""
        items = self._open_packed(indices, epoch) if self.pack is not None else self._open(indices, epoch)
        try:
            F, B = len(self.frame_ids), len(items)
            offsets, total = [0] * (F * B), 0
            for f in range(F):
                for b, it in enumerate(items):
                    offsets[f * B + b] = total
                    total += _padded(it.size)
            if self.pack is not None:
                return self._stage_packed(items, offsets, total, slot)
            if self.device_decode:
                return self._stage_compressed(items, offsets, total, slot)
            buf, spill = self._pinned[slot], None
            if buf is None or buf.numel() < total:
                host = spill = np.empty(total, dtype=np.uint8)
            else:
                host = buf.numpy()

            def decode(n):
                arr = self.dataset.decode(items[n % B].images[n // B])
                host[offsets[n]:offsets[n] + arr.size] = arr.reshape(-1)

            self._map(decode, range(F * B))
        finally:
            for it in items:
                it.close()
        return _Staged(slot, total, offsets, items, spill)

    def _stage_compressed(self, items, offsets, frames_total: int, slot: int) -> _Staged:
        """Step 3 with device_decode: the staging block holds the decoder's tables and the
        unstuffed streams, then the frames PIL had to decode.  Host work only."""
        F, B = len(self.frame_ids), len(items)

        def load(n):
            it = items[n % B]
            with open(it.paths[n // B], "rb") as f:
                data = f.read()
            s = jpeg_ops.parse_jpeg(data)
            if s is None and self.device_png:
                s = png_ops.parse_png(data)
            if s is not None and (s.height, s.width) == it.size:
                return s
            return self.dataset.decode(it.images[n // B])

        got = self._map(load, range(F * B))
        on_device = [n for n in range(F * B) if isinstance(got[n], jpeg_ops.JpegStream)]
        as_png = [n for n in range(F * B) if isinstance(got[n], png_ops.PngStream)]
        streams = [got[n] for n in on_device]
        images, quant, huff, base, pos = None, [], [], 0, 0
        if streams:
            images, quant, huff, base, pos = jpeg_ops.describe_batch(streams, [offsets[n] for n in on_device])
            jpeg_ops.check_described(images, len(streams), len(quant), len(huff), pos - base, frames_total)
        jtotal, pil, png = pos, [], None
        if as_png:   # their own region behind the JPEG one
            pos = (pos + ALIGN - 1) // ALIGN * ALIGN
            pstreams = [got[n] for n in as_png]
            pimages, pbase, ptotal = png_ops.describe_png_batch(pstreams, [offsets[n] for n in as_png])
            png_ops.check_png_described(pimages, len(pstreams), ptotal - pbase, frames_total)
            png = _StagedPng(pimages, len(pstreams), pos, pbase, ptotal)
            pos += ptotal
        for n in range(F * B):
            if not isinstance(got[n], (jpeg_ops.JpegStream, png_ops.PngStream)):
                pos = (pos + ALIGN - 1) // ALIGN * ALIGN
                pil.append((n, pos, got[n].size))
                pos += got[n].size
        total = max(pos, 16)
        buf, spill = self._pinned[slot], None
        if buf is None or buf.numel() < total:
            host = spill = np.empty(total, dtype=np.uint8)
        else:
            host = buf.numpy()
        if streams:
            jpeg_ops.fill_staging(host, streams, images, quant, huff, base)
        if png is not None:
            png_ops.fill_png_staging(host[png.offset:png.offset + png.total], pstreams, png.images, png.base)
        for n, o, size in pil:
            host[o:o + size] = got[n].reshape(-1)
        self.pil_fallbacks += len(pil)
        names = [(items[n % B].index, items[n % B].line, items[n % B].paths[n // B], "jpeg") for n in on_device]
        names += [(items[n % B].index, items[n % B].line, items[n % B].paths[n // B], "png") for n in as_png]
        st = _Staged(slot, total, offsets, items, spill)
        st.jpeg = _StagedJpeg(images, len(streams), len(quant), len(huff), base, jtotal, pil, frames_total, names)
        st.jpeg.png = png
        return st

    def _stage_packed(self, items, offsets, frames_total: int, slot: int) -> _Staged:
        """Step 3 from a pack: this (producer) thread lays out the block and gathers the table
        bank from the records' ids; the decoding threads read every record into its place.
        Host work only, and no byte of a stream is touched by the interpreter."""
        F, B = len(self.frame_ids), len(items)
        pack = self.pack
        recs = pack.records
        rows = [items[n % B].rows[n // B] for n in range(F * B)]
        on_device = [n for n in range(F * B) if recs["kind"][rows[n]] == KIND_JPEG]
        nj = len(on_device)
        images = (_lib.JpegImage * max(nj, 1))()
        index_offsets = (ctypes.c_uint64 * max(nj, 1))()
        quant: Dict[int, int] = {}
        huff: Dict[int, int] = {}
        pos, reads = 0, []          # reads: (row, offset behind the tables or in the block, bytes)
        for i, n in enumerate(on_device):
            r = recs[rows[n]]
            im = images[i]
            im.height, im.width, im.sampling = int(r["height"]), int(r["width"]), int(r["sampling"])
            im.out_offset, im.stream_bytes, im.stream_offset = offsets[n], int(r["stream_bytes"]), pos
            for c in range(3):
                im.quant[c] = quant.setdefault(int(r["quant"][c]), len(quant))
                im.dc[c] = huff.setdefault(int(r["dc"][c]), len(huff))
                im.ac[c] = huff.setdefault(int(r["ac"][c]), len(huff))
            index_offsets[i] = pos + (im.stream_bytes + 15) // 16 * 16
            reads.append((rows[n], pos, int(r["data_bytes"])))
            pos += (int(r["data_bytes"]) + 15) // 16 * 16
        if len(quant) > 255 or len(huff) > 255:
            raise ValueError("more than 255 distinct tables in one batch: use a smaller batch")
        nq, nh = len(quant) * _lib.JPEG_QUANT_BYTES, len(huff) * _lib.JPEG_HUFF_BYTES
        base = (nq + nh + 15) // 16 * 16
        jtotal = (base + max(pos, 16)) if nj else 0
        if nj:
            jpeg_ops.check_described_indexed(images, index_offsets, nj, len(quant), len(huff), jtotal - base,
                                             frames_total)
        reads = [(row, base + o, b) for row, o, b in reads]
        pos, pil, png = jtotal, [], None
        as_png = [n for n in range(F * B) if recs["kind"][rows[n]] == KIND_PNG]
        if as_png:   # their own region behind the JPEG one: the image array, the index offsets, the records
            pos = (pos + ALIGN - 1) // ALIGN * ALIGN
            npng = len(as_png)
            pimages = (_lib.PngImage * npng)()
            pindex = (ctypes.c_uint64 * npng)()
            pbase = (npng * (png_ops.IMAGE_BYTES + 8) + 15) // 16 * 16
            o = 0
            for i, n in enumerate(as_png):
                r = recs[rows[n]]
                im = pimages[i]
                im.height, im.width, im.out_offset = int(r["height"]), int(r["width"]), offsets[n]
                im.stream_offset, im.stream_bytes = o, int(r["stream_bytes"])
                pindex[i] = o + (im.stream_bytes + 15) // 16 * 16
                reads.append((rows[n], pos + pbase + o, int(r["data_bytes"])))   # one preadv: the index behind the stream
                o += (int(r["data_bytes"]) + 15) // 16 * 16
            ptotal = pbase + max(o, 16)
            png_ops.check_png_described_indexed(pimages, pindex, npng, pack.png_segment_bytes, ptotal - pbase,
                                                frames_total)
            png = _StagedPng(pimages, npng, pos, pbase, ptotal)
            png.index_offsets, png.segment_bytes = pindex, pack.png_segment_bytes
            pos += ptotal
        for n in range(F * B):
            if recs["kind"][rows[n]] not in (KIND_JPEG, KIND_PNG):
                pos = (pos + ALIGN - 1) // ALIGN * ALIGN
                size = int(recs["data_bytes"][rows[n]])
                pil.append((n, pos, size))
                reads.append((rows[n], pos, size))
                pos += size
        total = max(pos, 16)
        buf, spill = self._pinned[slot], None
        if buf is None or buf.numel() < total:
            host = spill = np.empty(total, dtype=np.uint8)
        else:
            host = buf.numpy()
        if nj:
            host[:nq] = pack.quant[list(quant)].reshape(-1)
            host[nq:nq + nh] = pack.huff[list(huff)].reshape(-1)
        if png is not None:
            nb = png.n * png_ops.IMAGE_BYTES
            head = host[png.offset:png.offset + png.base]
            head[:nb] = np.frombuffer(png.images, np.uint8, nb)
            head[nb:nb + 8 * png.n] = np.frombuffer(png.index_offsets, np.uint8, 8 * png.n)
            head[nb + 8 * png.n:] = 0
        self._map(lambda rd: pack.read_into(rd[0], host[rd[1]:rd[1] + rd[2]]), reads)
        names = [(items[n % B].index, items[n % B].line, items[n % B].paths[n // B], "jpeg") for n in on_device]
        names += [(items[n % B].index, items[n % B].line, items[n % B].paths[n // B], "png") for n in as_png]
        st = _Staged(slot, total, offsets, items, spill)
        st.jpeg = _StagedJpeg(images, nj, len(quant), len(huff), base, jtotal, pil, frames_total, names)
        st.jpeg.index_offsets = index_offsets
        st.jpeg.png = png
        return st

    def _reserve(self, slot: int, total: int):
        """Slot `slot`'s pinned buffer holds `total` bytes (caller's thread; the slot is free)."""
        buf = self._pinned[slot]
        if buf is None or buf.numel() < total:
            self._pinned[slot] = torch.empty(total + total // 8, dtype=torch.uint8, pin_memory=True)

    def _finish(self, st: _Staged) -> Dict:
        """Step 4, on the caller's thread and stream."""
        with torch.cuda.device(self.device):
            if st.spill is not None:
                self._reserve(st.slot, st.total)
                self._pinned[st.slot].numpy()[:st.total] = st.spill
            dev = torch.empty(st.total, dtype=torch.uint8, device=self.device)
            dev.copy_(self._pinned[st.slot][:st.total], non_blocking=True)
            self.uploaded_bytes += st.total
            if st.jpeg is not None:
                dev = self._decode_on_device(st, dev)
            if self._uploaded[st.slot] is None:
                self._uploaded[st.slot] = torch.cuda.Event()
            self._uploaded[st.slot].record()
            draws = [it.draw for it in st.items]
            sides = [it.side for it in st.items] if "s" in self.frame_ids else None
            inputs = self._aug_for(len(st.items))(dev, [it.size for it in st.items], st.offsets, draws, sides)
            if self.with_depth:
                inputs["depth_gt"] = self.dataset.get_depths(st.items, device=self.device).unsqueeze(1)
        return inputs

    def _decode_on_device(self, st: _Staged, up: torch.Tensor) -> torch.Tensor:
        """The ragged frame buffer of a device-decoded batch from its uploaded staging block
        `up`: the decoder's launches, the device copies of the PIL-decoded frames, and the
        status words on their way to the slot's pinned copy (all on the caller's stream,
        before the slot's event is recorded)."""
        j = st.jpeg
        frames = torch.empty(j.frames_total, dtype=torch.uint8, device=self.device)
        words = j.n + (j.png.n if j.png is not None else 0)
        if words:
            host = self._status[st.slot]
            if host is None or host.numel() < words:
                host = self._status[st.slot] = torch.empty(max(words, len(self.frame_ids) * self.batch_size),
                                                           dtype=torch.int32, pin_memory=True)
            self._status_of[st.slot] = j.names   # the JPEG streams' words, then the PNG streams'
        if j.n:
            if j.index_offsets is not None:
                status = jpeg_ops.run_staged_indexed(up, j.images, j.index_offsets, j.n, j.num_quant, j.num_huff,
                                                     j.base, j.jtotal, frames, self.device)
            else:
                status = jpeg_ops.run_staged(up, j.images, j.n, j.num_quant, j.num_huff, j.base, j.jtotal, frames,
                                             self.device)
            host[:j.n].copy_(status, non_blocking=True)
        if j.png is not None:
            p = j.png
            if p.index_offsets is not None:
                status = png_ops.run_png_staged_indexed(up[p.offset:p.offset + p.total], p.images, p.index_offsets,
                                                        p.n, p.base, p.total, p.segment_bytes, frames, self.device)
            else:
                status = png_ops.run_png_staged(up[p.offset:p.offset + p.total], p.images, p.n, p.base, p.total,
                                                frames, self.device)
            host[j.n:words].copy_(status, non_blocking=True)
        for n, o, size in j.pil:
            frames[st.offsets[n]:st.offsets[n] + size].copy_(up[o:o + size], non_blocking=True)
        return frames

    def _check_status(self, slot: int):
        """After slot `slot`'s event: raises if one of its streams did not decode."""
        names, self._status_of[slot] = self._status_of[slot], None
        if not names:
            return
        words = self._status[slot][:len(names)].tolist()
        bad = [(w, name) for w, name in zip(words, names) if w]
        if bad:
            w, (index, line, path, kind) = bad[0]
            why = (png_ops.status_text(w) if kind == "png"
                   else "the pack's synchronisation index does not fit the stream, or the stream does not hold the "
                   "image's blocks" if w & _lib.JPEG_ST_INDEX
                   else "the entropy-coded data does not hold the image's blocks")
            raise RuntimeError(f"split line {index} ({line!r}): {path} did not decode on the device (status {w}: "
                               f"{why}); {len(bad)} bad file(s) in its batch")

    # -------------------------------------------------------------- iteration
    def __iter__(self) -> Iterator[Dict]:
        epoch = self.epoch
        todo = self.batches(epoch)
        if not todo:
            self.epoch = epoch + 1
            return
        # every slot is free once the uploads of an earlier epoch have run; the ring is
        # sized here, before the producer starts, from the first batch's headers
        first = self._open_packed(todo[0], epoch) if self.pack is not None else self._open(todo[0], epoch)
        for it in first:
            it.close()
        need = len(self.frame_ids) * sum(_padded(it.size) for it in first)
        free: "queue.Queue" = queue.Queue()
        for slot in range(self._ring):
            if self._uploaded[slot] is not None:
                self._uploaded[slot].synchronize()
            self._status_of[slot] = None   # an epoch that was abandoned: its words are not this one's
            self._reserve(slot, need)
            free.put(slot)
        in_flight = collections.deque()   # slots behind an upload, oldest first

        def retire(keep: int = IN_FLIGHT):
            while len(in_flight) >= max(keep, 1):
                slot = in_flight.popleft()
                self._uploaded[slot].synchronize()   # its upload has run: the producer may refill it
                self._check_status(slot)
                free.put(slot)

        if self._pool is None:   # no threads: everything on the caller's thread
            for indices in todo:
                retire()
                st = self._stage(indices, epoch, free.get_nowait())
                out = self._finish(st)
                in_flight.append(st.slot)
                yield out
            if self.device_decode:
                retire(0)   # the last batches' status words, before the epoch ends
            self.epoch = epoch + 1
            return
        ready: "queue.Queue" = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def put(obj):
            while not stop.is_set():
                try:
                    ready.put(obj, timeout=0.1)
                    return
                except queue.Full:
                    pass

        def take():
            while not stop.is_set():
                try:
                    return free.get(timeout=0.1)
                except queue.Empty:
                    pass
            return None

        def produce():   # host work only: no call into the HIP runtime on this thread
            try:
                for indices in todo:
                    slot = take()
                    if slot is None:
                        return
                    put(self._stage(indices, epoch, slot))
            except BaseException as e:   # handed to the consumer
                put(e)

        producer = threading.Thread(target=produce, name="md2-loader", daemon=True)
        producer.start()
        try:
            for _ in todo:
                retire()
                st = ready.get()
                if isinstance(st, BaseException):
                    raise st
                out = self._finish(st)
                in_flight.append(st.slot)
                yield out
            if self.device_decode:
                retire(0)
            self.epoch = epoch + 1
        finally:
            stop.set()
            producer.join()

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
