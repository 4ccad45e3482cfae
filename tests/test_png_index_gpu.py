"""The indexed PNG decoder on the device (md2_png_index, md2_png_run_indexed):
the device's index against the pure-Python restatement byte for byte, the indexed decode
against the serial one and Pillow on the libraries' streams, on frames with and without a
boundary and on hand-made streams whose matches reach across segment boundaries; damaged
indexes in the middle of a batch (their own status word, neighbours and every guard byte
untouched); a stream damaged behind its index; two runs; one hipGraph capture.  S = 1024 and
frames of a few KB throughout: 7 or 8 segments each."""
import io
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import png_case as pc
import png_index_case as pic

pytestmark = pytest.mark.gpu

S = pic.S
GUARD = 64
ST_STAGE, ST_ADLER, ST_INDEX = 1 | 2 | 4 | 8, 32, 64


def pillow(png):
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))


def layout(streams):
    """Frame offsets (multiples of 16) with at least GUARD bytes before, between and behind."""
    offsets, pos = [], GUARD
    for s in streams:
        offsets.append(pos)
        pos = (pos + s.height * s.width * 3 + GUARD + 15) // 16 * 16
    return offsets, pos


def frames_of(out, streams, offsets, fill=0xA5):
    """The frames of `out` and a check that no byte outside them was written."""
    host = out.cpu().numpy()
    keep = np.ones(host.size, bool)
    frames = []
    for s, o in zip(streams, offsets):
        n = s.height * s.width * 3
        keep[o:o + n] = False
        frames.append(host[o:o + n].reshape(s.height, s.width, 3).copy())
    assert (host[keep] == fill).all(), "a byte outside the frames was written"
    return frames


def parsed(pngs):
    from monodepth2_amd.png_ops import parse_png
    streams = [parse_png(p) for p in pngs]
    assert all(s is not None for s in streams)
    return streams


def decode_both(pngs, indexes=None):
    """(frames, status) of the indexed decode and of the serial one, guards checked; the
    indexes are the device's unless given."""
    from monodepth2_amd.png_ops import decode_png_batch, decode_png_batch_indexed, index_png_batch
    streams = parsed(pngs)
    if indexes is None:
        indexes = index_png_batch(streams, S)
    offsets, total = layout(streams)
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    status = decode_png_batch_indexed(streams, indexes, out, offsets).cpu().tolist()
    indexed = (frames_of(out, streams, offsets), status)
    out.fill_(0xA5)
    status = decode_png_batch(streams, out, offsets).cpu().tolist()
    return indexed, (frames_of(out, streams, offsets), status), indexes, streams


def assert_parity(cases):
    """For {name: png}: the device index is the restatement's, the indexed decode is the
    serial one is Pillow, every status 0.  One batch."""
    names = list(cases)
    pngs = [cases[n] for n in names]
    (fi, si), (fs, ss), indexes, streams = decode_both(pngs)
    for k, name in enumerate(names):
        want, walk = pic.index_of(streams[k], S)
        assert np.array_equal(indexes[k], want), (name, pic.read_index(indexes[k]), walk.entries)
        assert si[k] == 0 and ss[k] == 0, (name, si[k], ss[k])
        assert np.array_equal(fi[k], fs[k]) and np.array_equal(fi[k], pillow(pngs[k])), name
    return {n: pic.index_of(streams[k], S)[1] for k, n in enumerate(names)}


# ------------------------------------------------------------------ parity
def test_the_libraries_streams():
    walks = assert_parity(pic.library_cases())
    for name, w in walks.items():
        if name != "1x1":
            assert len(w.entries) >= 3, (name, len(w.entries))     # not one segment by accident
    assert any(w.crossing for w in walks.values())


def test_hand_made_streams_reach_across_boundaries():
    cases = pic.handmade_cases()
    cases["far"] = pic.far_case()
    walks = assert_parity(cases)
    for name, w in walks.items():
        assert len(w.entries) >= 3 and w.crossing >= 1, (name, len(w.entries), w.crossing)
    assert walks["chain_through_segments"].depth >= 2


def test_a_batch_of_mixed_sizes():
    pngs = pic.mixed_batch()
    assert len(pngs) >= 8
    walks = assert_parity({"mixed%d" % i: p for i, p in enumerate(pngs)})
    counts = sorted(len(w.entries) for w in walks.values())
    assert counts[0] == 1 and counts[-1] >= 8          # frames without a boundary next to frames with many
    assert all(c == 1 or c >= 3 for c in counts), counts


def test_other_segment_sizes_and_the_default():
    """Every other kernel instance: S = 2048, 4096, 8192 and 32768 on frames of four segments
    (and one of two at 2048), the default S on frames of 66 x 120 (two) and 130 x 100 (three)."""
    from monodepth2_amd.png_ops import SEGMENT_BYTES, decode_png_batch_indexed, index_png_batch, index_segment_bytes
    rng = np.random.default_rng(9)
    for s_bytes, sizes in ((2048, [(24, 100), (40, 33)]), (4096, [(40, 110)]), (8192, [(80, 110)]),
                           (SEGMENT_BYTES, [(66, 120), (130, 100)]), (32768, [(130, 280)])):
        pngs = [pc.write_png(pic._scene(rng, h, w), rng.integers(0, 5, h).tolist(), level=6) for h, w in sizes]
        streams = parsed(pngs)
        indexes = index_png_batch(streams, s_bytes)
        offsets, total = layout(streams)
        out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        status = decode_png_batch_indexed(streams, indexes, out, offsets).cpu().tolist()
        for k, f in enumerate(frames_of(out, streams, offsets)):
            want, _ = pic.index_of(streams[k], s_bytes)
            assert np.array_equal(indexes[k], want) and index_segment_bytes(indexes[k]) == s_bytes
            assert status[k] == 0 and np.array_equal(f, pillow(pngs[k]))
            assert pic.read_index(want)[0] >= (2 if (s_bytes, k) in ((2048, 1), (SEGMENT_BYTES, 0)) else 3)
    assert SEGMENT_BYTES == 16384


def test_two_runs_are_bit_equal():
    pngs = list(pic.handmade_cases().values())[:3] + pic.mixed_batch()[:3]
    (fa, sa), _, indexes, _ = decode_both(pngs)
    (fb, sb), _, again, _ = decode_both(pngs)
    assert sa == sb == [0] * len(pngs)
    assert all(np.array_equal(a, b) for a, b in zip(fa, fb))
    assert all(np.array_equal(a, b) for a, b in zip(indexes, again))


# ------------------------------------------------------------------ the call with the caller's buffers
class Direct:
    """md2_png_run_indexed with buffers of the test's own: `out` and the workspace between
    guard bytes, the staging block uploaded once."""

    def __init__(self, streams, indexes):
        from monodepth2_amd import _lib, png_ops
        self.L, self.lib = _lib.lib(), _lib
        self.streams, self.n = streams, len(streams)
        self.offsets, total = layout(streams)
        self.images, self.index_offsets, self.base, self.total = png_ops.describe_png_batch_indexed(
            streams, indexes, self.offsets, S)
        png_ops.check_png_described_indexed(self.images, self.index_offsets, self.n, S, self.total - self.base, total)
        host = np.zeros(self.total, np.uint8)
        png_ops.fill_png_staging_indexed(host, streams, indexes, self.images, self.index_offsets, self.base)
        self.block = torch.from_numpy(host).cuda()
        self.out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        self.need = self.L.md2_png_indexed_workspace_bytes(self.images, self.n, S)
        assert self.need > 0
        self.ws = torch.full((self.need + 2 * 256,), 0x5A, dtype=torch.uint8, device="cuda")
        self.status = torch.full((self.n + 2,), -1, dtype=torch.int32, device="cuda")

    def run(self):
        ptr = self.block.data_ptr()
        rc = self.L.md2_png_run_indexed(ptr + self.base, self.total - self.base, self.images, ptr, self.index_offsets,
                                        ptr + self.n * 32, self.n, S, self.ws.data_ptr() + 256, self.need,
                                        self.out.data_ptr(), self.out.numel(), self.status.data_ptr() + 4,
                                        self.lib.stream(self.out.device))
        assert rc == 0, self.L.md2_last_error()

    def result(self):
        """(frames, status words) with every guard checked."""
        torch.cuda.synchronize()
        ws = self.ws.cpu().numpy()
        assert (ws[:256] == 0x5A).all() and (ws[256 + self.need:] == 0x5A).all(), "the workspace's guards"
        st = self.status.cpu().tolist()
        assert st[0] == -1 and st[-1] == -1, "the status words' neighbours"
        return frames_of(self.out, self.streams, self.offsets), st[1:-1]


def small_pngs():
    rng = np.random.default_rng(17)
    return [pc.write_png(pic._scene(rng, pic.H, pic.W), rng.integers(0, 5, pic.H).tolist(), level=lv) for lv in (6, 9)]


def damage(index, walk, kind):
    """A copy of the index of a stream with the entries walk.entries, damaged."""
    n = len(walk.entries)
    assert n >= 4
    hb, sb, op = walk.entries[2]
    if kind == "out_pos+1":
        return pic.write_entry(index, 2, out_pos=op + 1)
    if kind == "out_pos-1":
        return pic.write_entry(index, 2, out_pos=op - 1)
    if kind == "symbol_bit+1":
        return pic.write_entry(index, 2, symbol_bit=sb + 1)
    if kind == "symbol_bit-1":
        return pic.write_entry(index, 2, symbol_bit=sb - 1)
    if kind == "other_block":
        other = next(e[0] for e in walk.entries if e[0] != hb)
        return pic.write_entry(index, 2, header_bit=other, symbol_bit=max(sb, other))
    if kind == "entry0_bits":          # segment 0 starts at bit 0, whatever else fits
        return pic.write_entry(index, 0, header_bit=0, symbol_bit=walk.entries[1][1])
    if kind == "header_bit+1":
        return pic.write_entry(index, 2, header_bit=hb + 1)
    out = np.array(index, copy=True)
    if kind in ("count+1", "count-1"):
        out[:4] = np.frombuffer(struct.pack("<I", n + (1 if kind == "count+1" else -1)), np.uint8)
    elif kind == "swapped":
        a, b = (slice(16 + 24 * k, 16 + 24 * (k + 1)) for k in (1, 2))
        out[a], out[b] = index[b].copy(), index[a].copy()
    elif kind == "zeros":
        out[:] = 0
    elif kind == "ones":
        out[:] = 255
    elif kind == "other_s":
        out[4:8] = np.frombuffer(struct.pack("<I", 2048), np.uint8)
    elif kind == "far_bits":
        return pic.write_entry(index, 2, header_bit=1 << 40, symbol_bit=1 << 41)
    else:
        raise ValueError(kind)
    return out


DAMAGES = ["out_pos+1", "out_pos-1", "symbol_bit+1", "symbol_bit-1", "other_block", "header_bit+1", "count+1",
           "count-1", "swapped", "zeros", "ones", "other_s", "far_bits", "entry0_bits"]


@pytest.fixture(scope="module")
def trio():
    """(pngs, streams, true indexes, the middle stream's walk): the middle stream has several
    blocks (sync flushes), so an entry can point into another one."""
    rng = np.random.default_rng(23)
    before, after = small_pngs()
    middle = pc.write_png(pic._scene(rng, pic.H, pic.W), rng.integers(0, 5, pic.H).tolist(), flush_every=1500,
                          flush_mode=2)
    pngs = [before, middle, after]
    streams = parsed(pngs)
    made = [pic.index_of(s, S) for s in streams]
    assert len({e[0] for e in made[1][1].entries}) >= 3          # entries in at least 3 blocks
    return pngs, streams, [m[0] for m in made], made[1][1]


@pytest.mark.parametrize("kind", DAMAGES)
def test_a_damaged_index_sets_its_own_status_and_writes_nothing_else(trio, kind):
    pngs, streams, indexes, walk = trio
    bad = damage(indexes[1], walk, kind)
    assert not np.array_equal(bad, indexes[1])
    d = Direct(streams, [indexes[0], bad, indexes[2]])
    d.run()
    frames, status = d.result()
    assert status[0] == 0 and status[2] == 0, status
    assert status[1] & (ST_INDEX | ST_STAGE) and not status[1] & ~(ST_INDEX | ST_STAGE), status
    assert np.array_equal(frames[0], pillow(pngs[0])) and np.array_equal(frames[2], pillow(pngs[2]))
    assert (frames[1] == 0xA5).all(), "a frame whose index does not fit was written"


def test_the_true_indexes_through_the_same_call(trio):
    pngs, streams, indexes, _ = trio
    d = Direct(streams, indexes)
    d.run()
    frames, status = d.result()
    assert status == [0, 0, 0]
    assert all(np.array_equal(f, pillow(p)) for f, p in zip(frames, pngs))


def test_a_stream_damaged_behind_its_index_is_not_trusted(trio):
    """a flipped bit in a literal of a stored block, and one in a Huffman block"""
    from monodepth2_amd.png_ops import PngStream
    pngs, streams, indexes, _ = trio
    rng = np.random.default_rng(29)
    img = pic._scene(rng, pic.H, pic.W)
    stored = parsed([pc.write_png(img, [0] * pic.H, level=0)])[0]
    huff = streams[1]
    for s, byte in ((stored, 5 + 3000), (huff, len(huff.data) // 2)):
        index, walk = pic.index_of(s, S)
        assert len(walk.entries) >= 3
        hurt = PngStream(s.height, s.width, pc.flip_bit(s.data, byte, 3))
        d = Direct([streams[0], hurt, streams[2]], [indexes[0], index, indexes[2]])
        d.run()
        frames, status = d.result()
        assert status[0] == 0 and status[2] == 0 and status[1] != 0, status
        assert status[1] & (ST_ADLER | ST_STAGE | ST_INDEX)
        assert np.array_equal(frames[0], pillow(pngs[0])) and np.array_equal(frames[2], pillow(pngs[2]))


def test_one_capture_replays_to_the_same_bytes(trio):
    pngs, streams, indexes, _ = trio
    d = Direct(streams, indexes)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d.run()                                   # no allocation, no synchronisation inside the call
    torch.cuda.current_stream().wait_stream(side)
    eager, status = d.result()
    assert status == [0, 0, 0]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.run()
    for _ in range(2):
        d.out.fill_(0xA5)
        d.status.fill_(-1)
        d.ws[256:256 + d.need].fill_(0)
        graph.replay()
        frames, status = d.result()
        assert status == [0, 0, 0]
        assert all(np.array_equal(a, b) for a, b in zip(frames, eager))
        assert all(np.array_equal(f, pillow(p)) for f, p in zip(frames, pngs))


def test_check_names_the_first_bad_index(trio):
    from monodepth2_amd.png_ops import decode_png_batch_indexed
    pngs, streams, indexes, walk = trio
    offsets, total = layout(streams)
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="stream index 1 did not decode.*segment index"):
        decode_png_batch_indexed(streams, [indexes[0], damage(indexes[1], walk, "zeros"), indexes[2]], out, offsets,
                                 check=True)


def test_the_indexer_reports_the_inflate_stage(trio):
    """a stream that does not inflate gets its status bit and an index nothing decodes from"""
    from monodepth2_amd.png_ops import PngStream, index_png_batch
    pngs, streams, indexes, _ = trio
    short = PngStream(streams[1].height, streams[1].width, streams[1].data[:len(streams[1].data) // 2])
    got = index_png_batch([streams[0], short, streams[2]], S, check=False)
    assert got[1] is None and np.array_equal(got[0], indexes[0]) and np.array_equal(got[2], indexes[2])
    with pytest.raises(RuntimeError, match="stream index 1 did not inflate"):
        index_png_batch([streams[0], short, streams[2]], S)
