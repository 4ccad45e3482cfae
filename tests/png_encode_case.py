"""The PNG encoder's format rules (csrc/pngenc.hip) restated in numpy and pure
Python, and the named cases of its tests.  `encode_np(frame, kind, segment_bytes)` is the file
the device has to write, byte for byte; `encode_info` also says what the rules made of the
frame (filters, tokens, block kinds, where every segment starts).  test_png_encode_host.py
holds this restatement to the PNG and zlib standards (Pillow opens the files, zlib inflates
the streams).  No torch and no tests in here."""
import heapq
import struct
import zlib

import numpy as np

import logpanel_case as lc

RGB8, GRAY16 = 0, 1
BPP = {RGB8: 3, GRAY16: 2}
SIGNATURE = b"\x89PNG\r\n\x1a\n"
PRIME = 4096            # input bytes before a segment whose positions are in the table at its start
HASH_BITS = 12
WINDOW = 32768
STEP = 64               # positions per step: one per lane
MIN_MATCH, MAX_MATCH = 3, 258
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
ADLER = 65521


# ------------------------------------------------------------------ scanlines and filters
def raw_rows(frame, kind):
    """(h, bpp * w) uint8: the unfiltered scanlines (16-bit samples big-endian)."""
    a = np.asarray(frame)
    if kind == RGB8:
        assert a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8, (a.shape, a.dtype)
        return np.ascontiguousarray(a).reshape(a.shape[0], -1)
    assert kind == GRAY16 and a.ndim == 2 and a.dtype in (np.int16, np.uint16), (a.shape, a.dtype)
    return np.ascontiguousarray(a).view(np.uint16).astype(">u2").view(np.uint8).reshape(a.shape[0], -1)


def residuals(rows, bpp):
    """(5, h, L) uint8: every row under None, Sub, Up, Average, Paeth (row 0: zeros above)."""
    cur = rows.astype(np.int32)
    a = np.zeros_like(cur)
    a[:, bpp:] = cur[:, :-bpp]
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[:, bpp:] = b[:, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return (np.stack([cur, cur - a, cur - b, cur - ((a + b) >> 1), cur - paeth]) & 255).astype(np.uint8)


def filter_rows(rows, bpp):
    """(filters, filtered stream): per row the filter of the least sum of |signed residual|
    (the filter byte not counted), ties to the lowest number."""
    res = residuals(rows, bpp)
    r = res.astype(np.int64)
    cost = np.where(r < 128, r, 256 - r).sum(axis=2)        # (5, h)
    filters = np.argmin(cost, axis=0)                        # the first minimum
    h = rows.shape[0]
    out = np.empty((h, 1 + rows.shape[1]), np.uint8)
    out[:, 0] = filters
    out[:, 1:] = res[filters, np.arange(h)]
    return filters.tolist(), out.tobytes()


def adler32_by_rows(stream, row_len):
    """The device's combine: per row s1 = sum b, s2 = sum (row_len - j) b_j, rows in order."""
    a, b = 1, 0
    wgt = np.arange(row_len, 0, -1, dtype=np.uint64)
    for r in range(len(stream) // row_len):
        row = np.frombuffer(stream, np.uint8, row_len, r * row_len).astype(np.uint64)
        s1, s2 = int(row.sum()), int((row * wgt).sum())
        b = (b + row_len * a + s2 % ADLER) % ADLER
        a = (a + s1 % ADLER) % ADLER
    return b << 16 | a


# ------------------------------------------------------------------ matches and the parse
def hash3(d, p):
    v = d[p] | d[p + 1] << 8 | d[p + 2] << 16
    return ((v * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def _common(d, c, p, limit):
    n = 0
    while n < limit and d[c + n] == d[p + n]:
        n += 1
    return n


def parse_segment(d, start, end):
    """The tokens of filtered bytes [start, end): an int is a literal, (length, distance) a
    match.  The table maps a hash to the largest position inserted so far; a step of 64
    positions looks up first (the table as the step before left it) and inserts afterwards."""
    total = len(d)
    table = {}
    for p in range(max(0, start - PRIME), start):
        if p + 3 <= total:
            table[hash3(d, p)] = p
    tokens = []
    nxt = start                                   # the first position no token covers yet
    for base in range(start, end, STEP):
        stop = min(base + STEP, end)
        found = {}
        for p in range(max(base, nxt), stop):     # lanes below the carry do not search
            best = (0, 0)
            if p + 3 <= end:
                limit = min(MAX_MATCH, end - p)
                if p >= 1:
                    best = (_common(d, p - 1, p, limit), 1)
                c = table.get(hash3(d, p))
                if c is not None and p - c <= WINDOW:
                    n = _common(d, c, p, limit)
                    if n > best[0]:               # a tie stays with distance 1
                        best = (n, p - c)
            found[p] = best
        for p in range(base, stop):
            if p + 3 <= total:
                table[hash3(d, p)] = p
        p = max(base, nxt)
        while p < stop:
            n, dist = found[p]
            if n >= MIN_MATCH:
                tokens.append((n, dist))
                p += n
            else:
                tokens.append(d[p])
                p += 1
        nxt = p
    return tokens


def length_symbol(n):
    """(symbol, extra bits, extra value) of a match length."""
    v = n - 3
    if v < 8:
        return 257 + v, 0, 0
    if n == 258:
        return 285, 0, 0
    eb = v.bit_length() - 3
    return 261 + 4 * eb + ((v >> eb) & 3), eb, v & ((1 << eb) - 1)


def distance_symbol(dist):
    v = dist - 1
    if v < 4:
        return v, 0, 0
    nb = v.bit_length() - 1
    return 2 * nb + ((v >> (nb - 1)) & 1), nb - 1, v & ((1 << (nb - 1)) - 1)


# ------------------------------------------------------------------ codes
def code_lengths(freq, limit):
    """Huffman code lengths of the counts, at most `limit` bits.  Fewer than two used symbols:
    the lowest-numbered unused symbols count 1 until two are used.  Nodes are keyed (count,
    index), leaves by their symbol and merged nodes numbered on from the alphabet's size; the
    two least keys merge.  A code longer than `limit`: every count c > 0 becomes (c + 1) >> 1
    and the construction starts again."""
    n = len(freq)
    f = list(freq)
    s = 0
    while sum(1 for x in f if x) < 2:
        if f[s] == 0:
            f[s] = 1
        s += 1
    while True:
        heap = [(c, i) for i, c in enumerate(f) if c]
        heapq.heapify(heap)
        parent = {}
        nodes = n
        while len(heap) > 1:
            c1, i1 = heapq.heappop(heap)
            c2, i2 = heapq.heappop(heap)
            parent[i1] = parent[i2] = nodes
            heapq.heappush(heap, (c1 + c2, nodes))
            nodes += 1
        root = nodes - 1
        lens = [0] * n
        for i, c in enumerate(f):
            if c:
                k = i
                while k != root:
                    k = parent[k]
                    lens[i] += 1
        if max(lens) <= limit:
            return lens
        f = [(c + 1) >> 1 if c else 0 for c in f]


def canonical(lens):
    """RFC 1951's codes, bit-reversed: ready for an LSB-first writer."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lens)
    for i, n in enumerate(lens):
        if n:
            out[i] = int(format(nxt[n], "0%db" % n)[::-1], 2)
            nxt[n] += 1
    return out


def run_length(seq):
    """[(symbol, extra bits, extra value)] of the code lengths: at index i a run of r equal
    values starts.  Zeros with r >= 3: 18 (r >= 11) or 17 for min(r, 138).  A value equal to
    the one before it with r >= 3: 16 for min(r, 6).  Else the value itself."""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            n = min(r, 138)
            out.append((18, 7, n - 11) if n >= 11 else (17, 3, n - 3))
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3:
            n = min(r, 6)
            out.append((16, 2, n - 3))
        else:
            n = 1
            out.append((v, 0, 0))
        i += n
    return out


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def encode_segment(d, start, end, final):
    """(bytes, info) of one segment: its block, then (not the last) the empty stored block."""
    n = end - start
    tokens = parse_segment(d, start, end)
    lit, dst = [0] * 286, [0] * 30
    extra = 0
    for t in tokens:
        if isinstance(t, tuple):
            s, eb, _ = length_symbol(t[0])
            lit[s] += 1
            s2, eb2, _ = distance_symbol(t[1])
            dst[s2] += 1
            extra += eb + eb2
        else:
            lit[t] += 1
    lit[256] = 1
    ll, dl = code_lengths(lit, 15), code_lengths(dst, 15)
    hlit = max(257, max(i for i in range(286) if ll[i]) + 1)
    hdist = max(1, max(i for i in range(30) if dl[i]) + 1)
    ops = run_length(ll[:hlit] + dl[:hdist])
    clf = [0] * 19
    for s, _, _ in ops:
        clf[s] += 1
    cl = code_lengths(clf, 7)
    hclen = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    bits = 3 + 14 + 3 * hclen + sum(cl[s] + eb for s, eb, _ in ops) + extra
    bits += sum(lit[i] * ll[i] for i in range(286)) + sum(dst[i] * dl[i] for i in range(30))
    stored = (bits + 7) // 8 >= n + 5
    w = Bits()
    if stored:
        w.put(int(final), 8)
        w.put(n, 16)
        w.put(n ^ 0xFFFF, 16)
        for k in range(start, end):
            w.put(d[k], 8)
    else:
        w.put(int(final) | 2 << 1, 3)
        w.put(hlit - 257, 5)
        w.put(hdist - 1, 5)
        w.put(hclen - 4, 4)
        for i in range(hclen):
            w.put(cl[CL_ORDER[i]], 3)
        clc = canonical(cl)
        for s, eb, ev in ops:
            w.put(clc[s], cl[s])
            w.put(ev, eb)
        lc_, dc = canonical(ll), canonical(dl)
        for t in tokens:
            if isinstance(t, tuple):
                s, eb, ev = length_symbol(t[0])
                w.put(lc_[s], ll[s])
                w.put(ev, eb)
                s, eb, ev = distance_symbol(t[1])
                w.put(dc[s], dl[s])
                w.put(ev, eb)
            else:
                w.put(lc_[t], ll[t])
        w.put(lc_[256], ll[256])
        assert w.n == bits, (w.n, bits)
    if not final:
        w.put(0, 3)
        w.align()
        w.put(0xFFFF0000, 32)
    info = dict(start=start, end=end, stored=stored, tokens=tokens, dist_symbols=sum(1 for x in dst if x),
                lit_symbols=sum(1 for x in lit if x))
    return w.bytes(), info


# ------------------------------------------------------------------ the file
def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def file_bytes(h, w, kind, zstream):
    ihdr = struct.pack(">IIBBBBB", w, h, 8 if kind == RGB8 else 16, 2 if kind == RGB8 else 0, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zstream) + chunk(b"IEND", b"")


def encode_bound(h, w, kind, segment_bytes):
    """Every block stored (n + 5), the flush behind every segment (5), header and trailer."""
    total = h * (1 + BPP[kind] * w)
    return total + 10 * (-(-total // segment_bytes)) + 6


def encode_info(frame, kind, segment_bytes=16384):
    rows = raw_rows(frame, kind)
    h, w = rows.shape[0], rows.shape[1] // BPP[kind]
    filters, d = filter_rows(rows, BPP[kind])
    total = len(d)
    parts, segments, pos = [], [], 2
    for start in range(0, total, segment_bytes):
        end = min(total, start + segment_bytes)
        b, info = encode_segment(d, start, end, end == total)
        info["offset"], info["nbytes"] = pos, len(b)
        pos += len(b)
        parts.append(b)
        segments.append(info)
    adler = adler32_by_rows(d, 1 + rows.shape[1])
    z = b"\x78\x01" + b"".join(parts) + struct.pack(">I", adler)
    return dict(file=file_bytes(h, w, kind, z), zstream=z, filtered=d, filters=filters, segments=segments,
                height=h, width=w, kind=kind, segment_bytes=segment_bytes)


def encode_np(frame, kind, segment_bytes=16384):
    return encode_info(frame, kind, segment_bytes)["file"]


# ------------------------------------------------------------------ cases
def _rgb_for_total(total_rows_bytes):
    """(h, w) of an RGB8 frame whose filtered size is exactly the argument."""
    for h in range(1, 200):
        if total_rows_bytes % h == 0 and (total_rows_bytes // h - 1) % 3 == 0 and total_rows_bytes // h > 1:
            return h, (total_rows_bytes // h - 1) // 3
    raise AssertionError(total_rows_bytes)


def _scene(rng, h, w):
    """Smooth columns, a noisy band and a far repeat: literals and matches near and far."""
    x = np.arange(w)[None, :, None]
    y = np.arange(h)[:, None, None]
    img = ((x * 3 + y * 2 + np.arange(3)[None, None, :] * 40) & 255).astype(np.uint8) + np.zeros((h, w, 3), np.uint8)
    if h >= 4:
        img[h // 4:h // 2] = rng.integers(0, 256, (h // 2 - h // 4, w, 3), dtype=np.uint8)
        img[-(h // 4):] = img[h // 4:h // 4 + h // 4]
    return img


def filters_5rows():
    """Five rows of 16 RGB pixels on which None, Sub, Up, Average and Paeth win in turn."""
    rng = np.random.default_rng(21)
    w = 16
    img = np.zeros((5, w, 3), np.int64)
    img[0] = np.where(np.arange(w)[:, None] & 1, 251, 5)                  # +5, -5, ...: None (ties with Up)
    img[1] = 100                                                          # a flat row far from row 0: Sub
    img[2] = img[1] + 3 * (np.arange(w)[:, None] & 1)                     # the row above plus 0, 3, 0, 3: Up
    left = np.zeros((w, 3), np.int64)                                     # each pixel the mean of left and above
    row = np.zeros((w, 3), np.int64)
    for x in range(w):
        row[x] = (left + img[2, x]) // 2 if x else img[2, x] // 2
        left = row[x]
    img[3] = row
    img[4] = img[3]                                                       # Paeth: a + b - c on a diagonal ramp
    for x in range(w):
        a = img[4, x - 1] if x else np.zeros(3, np.int64)
        b = img[3, x]
        c = img[3, x - 1] if x else np.zeros(3, np.int64)
        p = a + b - c
        cand = np.stack([a, b, c])
        pick = np.argmin(np.abs(cand - p), axis=0)
        img[4, x] = cand[pick, np.arange(3)] + (1 if x % 5 == 2 else 0)
    return (img & 255).astype(np.uint8)


def cases():
    """name -> [(frame, kind, segment_bytes)]: one entry but for mixed_batch."""
    rng = np.random.default_rng(7)
    out = {}
    out["one_1x1_rgb"] = [(np.array([[[200, 3, 77]]], np.uint8), RGB8, 16384)]
    g = np.array([0, 1, 255, 256, 32767, 32768, 65535, 0, 65535, 256, 1, 32768, 255, 32767, 0], np.uint16)
    out["gray16_3x5"] = [(g.reshape(3, 5).view(np.int16), GRAY16, 16384)]
    out["filters_5rows_rgb"] = [(filters_5rows(), RGB8, 16384)]
    tie = np.zeros((2, 6, 3), np.uint8)
    tie[0] = 7                      # row 0: Sub and Paeth tie (no row above); row 1: Up, Paeth tie
    tie[1] = 7
    out["tie_rows"] = [(tie, RGB8, 16384)]
    out["flat_40x70_rgb"] = [(np.zeros((40, 70, 3), np.uint8), RGB8, 16384)]
    out["noise_32x48_rgb"] = [(rng.integers(0, 256, (32, 48, 3), dtype=np.uint8), RGB8, 1024)]
    for name, total in (("exact_S", 1024), ("S_minus_1", 1023), ("S_plus_1", 1025), ("3S_plus_7", 3 * 1024 + 7)):
        h, w = _rgb_for_total(total)
        out["edge_" + name] = [(_scene(rng, h, w), RGB8, 1024)]
    out["row_straddles_cut"] = [(_scene(rng, 9, 100), RGB8, 1024)]           # rows of 301 bytes
    out["match_from_previous_segment"] = [(np.full((8, 120, 3), 33, np.uint8), RGB8, 1024)]
    disp = np.linspace(0.05, 0.6, 96, dtype=np.float64)[None, :] + np.linspace(0.0, 0.3, 64)[:, None]
    depth = np.clip(5.4 / disp, 0, 80.0) * 256
    out["depth_like_64x96_gray16"] = [(depth.astype(np.uint16).view(np.int16), GRAY16, 16384)]
    dc = lc.disp_cases()
    x = np.linspace(0, 1, 80, dtype=np.float32)[None, None, :]
    y = np.linspace(0, 1, 24, dtype=np.float32)[None, :, None]
    colour = np.concatenate([x + 0 * y, y + 0 * x, (x + y) / 2]).astype(np.float32)
    tiles = [(lc.COLOR, 0, (0, 0, 24, 80), colour), (lc.DISP, 0, (0, 80, 24, 80), dc["noise_24x80"]),
             (lc.DISP, 0, (24, 0, 24, 80), (x[0] * y[0] + 0.01).astype(np.float32)),
             (lc.MAP, 0, (24, 80, 24, 80), (dc["noise_24x80"] > 0.5).astype(np.float32))]
    out["panel_like_48x160_rgb"] = [(lc.build_sheet(1, 48, 160, tiles)[0], RGB8, 16384)]
    out["mixed_batch"] = [(_scene(rng, 20, 33), RGB8, 1024), (out["depth_like_64x96_gray16"][0][0], GRAY16, 4096),
                          (np.array([[[1, 2, 3]]], np.uint8), RGB8, 1024),
                          (rng.integers(0, 4, (7, 300), dtype=np.uint16) * 257, GRAY16, 1024),
                          (out["panel_like_48x160_rgb"][0][0], RGB8, 4096)]
    return out


COMPRESSIBLE = ("flat_40x70_rgb", "depth_like_64x96_gray16", "panel_like_48x160_rgb", "match_from_previous_segment",
                "edge_3S_plus_7", "row_straddles_cut")
