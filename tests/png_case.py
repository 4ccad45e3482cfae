"""PNG files made to order for the device decoder's tests (monodepth2_amd/png_ops.py,
csrc/png.hip): a writer that forces a filter per row (the filtering is done here, in Python),
takes zlib's level, strategy, window and flush points, splits the IDAT payload anywhere and
adds chunks; a bit writer for deflate blocks by hand (stored and fixed-Huffman, from literals
and (length, distance) tokens); a walk of a deflate stream's first block header; and ways to
damage a file.  No tests in here."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
NONE, SUB, UP, AVG, PAETH = range(5)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ------------------------------------------------------------------ filtering
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(img, filters):
    """The raw scanlines (filter byte + filtered bytes per row) of an (h, w, 3) uint8 image
    with filters[r] forced on row r (bpp = 3; row -1 and the pixels left of the row are 0)."""
    img = np.asarray(img, dtype=np.uint8)
    h, w, _ = img.shape
    flat = img.reshape(h, 3 * w).astype(np.int64)
    out = bytearray()
    zero = np.zeros(3 * w, np.int64)
    for r in range(h):
        cur, up = flat[r], (flat[r - 1] if r else zero)
        left = np.concatenate([np.zeros(3, np.int64), cur[:-3]])
        upleft = np.concatenate([np.zeros(3, np.int64), up[:-3]])
        f = int(filters[r])
        if f == NONE:
            pred = zero
        elif f == SUB:
            pred = left
        elif f == UP:
            pred = up
        elif f == AVG:
            pred = (left + up) >> 1
        elif f == PAETH:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, upleft)], np.int64)
        else:
            raise ValueError(f)
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


# ------------------------------------------------------------------ the container
def chunk(kind, payload=b""):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def ihdr(h, w, depth=8, colour=2, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))


def png_bytes(h, w, zstream, splits=(), extra=(), iend=True):
    """The file around a zlib stream: IHDR, the `extra` chunks, IDAT chunks of the sizes in
    `splits` (0 allowed) and one of the rest, IEND."""
    out = [SIGNATURE, ihdr(h, w)] + list(extra)
    pos = 0
    for n in splits:
        out.append(chunk(b"IDAT", zstream[pos:pos + n]))
        pos += n
    out.append(chunk(b"IDAT", zstream[pos:]))
    if iend:
        out.append(chunk(b"IEND"))
    return b"".join(out)


def zlib_stream(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_every=None, flush_mode=None):
    """zlib's stream of `raw`; with flush_every, a flush of flush_mode after every so many bytes."""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if flush_every is None:
        return c.compress(raw) + c.flush()
    out = []
    for i in range(0, len(raw), flush_every):
        out.append(c.compress(raw[i:i + flush_every]))
        out.append(c.flush(flush_mode))
    out.append(c.flush())
    return b"".join(out)


def write_png(img, filters=None, splits=(), extra=(), **zkw):
    """The PNG file of an (h, w, 3) uint8 image: filters[r] per row (default None everywhere),
    zlib_stream's keywords, png_bytes's splits and extra chunks."""
    img = np.asarray(img, dtype=np.uint8)
    h, w, _ = img.shape
    raw = filter_rows(img, [NONE] * h if filters is None else filters)
    return png_bytes(h, w, zlib_stream(raw, **zkw), splits, extra)


def image_of_raw(raw, h, w):
    """An (h, w, 3) image whose scanlines with filter None everywhere, but the filter bytes
    taken from `raw`, are `raw` — only for raw bytes whose filter bytes are all 0."""
    a = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert not a[:, 0].any()
    return a[:, 1:].reshape(h, w, 3).copy()


# ------------------------------------------------------------------ deflate by hand
def length_symbol(length):
    return 28 if length == 258 else max(i for i, b in enumerate(LEN_BASE) if b <= length)


def distance_symbol(distance):
    return max(i for i, b in enumerate(DIST_BASE) if b <= distance)


def canonical_codes(lens):
    """{symbol: code} of a list of code lengths (0 = unused), as RFC 1951 assigns them."""
    code, out = 0, {}
    for length in range(1, 16):
        for sym, n in enumerate(lens):
            if n == length:
                out[sym] = code
                code += 1
        code <<= 1
    return out


class BitWriter:
    """Bits LSB first, as deflate packs them; Huffman codes go in MSB first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, count):
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):
        self.bits(int(format(value, "0{}b".format(count))[::-1], 2), count)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)

    # fixed-Huffman symbols
    def literal_or_length(self, sym):
        if sym < 144:
            self.code(0x30 + sym, 8)
        elif sym < 256:
            self.code(0x190 + sym - 144, 9)
        elif sym < 280:
            self.code(sym - 256, 7)
        else:
            self.code(0xC0 + sym - 280, 8)

    def match(self, length, distance):
        ls, ds = length_symbol(length), distance_symbol(distance)
        self.literal_or_length(257 + ls)
        self.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
        self.code(ds, 5)
        self.bits(distance - DIST_BASE[ds], DIST_EXTRA[ds])

    def fixed_block(self, tokens, final=True, end=True):
        """A fixed-Huffman block of tokens: an int is a literal, a (length, distance) pair a match."""
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        for t in tokens:
            if isinstance(t, tuple):
                self.match(*t)
            else:
                self.literal_or_length(int(t))
        if end:
            self.literal_or_length(256)

    def stored_block(self, data, final=True, nlen=None):
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.align()
        self.bits(len(data), 16)
        self.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += data

    def dynamic_block(self, tokens, lit_lens, dist_lens, length_ops, final=True):
        """A dynamic-Huffman block of tokens.  lit_lens and dist_lens: the code lengths, up to
        the last symbol sent (at least 257 and 1 long).  length_ops: how they are sent, an int
        0..15 for one length or (16 | 17 | 18, repeat count); they must expand to lit_lens +
        dist_lens.  The code-length code is fixed and complete: 4 bits for 0..12, 5 for 13..18."""
        sent = []
        for op in length_ops:
            if isinstance(op, tuple):
                sent += [sent[-1] if op[0] == 16 else 0] * op[1]
            else:
                sent.append(op)
        assert sent == list(lit_lens) + list(dist_lens), "length_ops do not spell the lengths"
        cl = [4] * 13 + [5] * 6
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(len(lit_lens) - 257, 5)
        self.bits(len(dist_lens) - 1, 5)
        self.bits(19 - 4, 4)
        for s in CL_ORDER:
            self.bits(cl[s], 3)
        cl_codes = canonical_codes(cl)
        for op in length_ops:
            sym, rep = op if isinstance(op, tuple) else (op, None)
            self.code(cl_codes[sym], cl[sym])
            if sym == 16:
                self.bits(rep - 3, 2)
            elif sym == 17:
                self.bits(rep - 3, 3)
            elif sym == 18:
                self.bits(rep - 11, 7)
        lit_codes, dist_codes = canonical_codes(lit_lens), canonical_codes(dist_lens)
        for t in list(tokens) + [256]:
            if isinstance(t, tuple):
                ls, ds = length_symbol(t[0]), distance_symbol(t[1])
                self.code(lit_codes[257 + ls], lit_lens[257 + ls])
                self.bits(t[0] - LEN_BASE[ls], LEN_EXTRA[ls])
                self.code(dist_codes[ds], dist_lens[ds])
                self.bits(t[1] - DIST_BASE[ds], DIST_EXTRA[ds])
            else:
                self.code(lit_codes[int(t)], lit_lens[int(t)])

    def block_header(self, btype, final=True):
        self.bits(1 if final else 0, 1)
        self.bits(btype, 2)


def settle_filter_bytes(tokens, row_bytes, rng):
    """Sets the literals that end up at row starts (directly or through matches) to 0..4, so
    that what the tokens inflate to is a valid set of scanlines.  In place; returns tokens."""
    source = []   # per output byte: the token index of the literal it is a copy of
    for k, t in enumerate(tokens):
        if isinstance(t, tuple):
            for _ in range(t[0]):
                source.append(source[-t[1]])
        else:
            source.append(k)
    for p in range(0, len(source), row_bytes):
        tokens[source[p]] = int(rng.integers(0, 5))
    return tokens


def expand(tokens, prefix=b""):
    """The bytes a token list inflates to (behind `prefix`, which matches may reach into)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, tuple):
            length, distance = t
            assert distance <= len(out)
            for _ in range(length):
                out.append(out[-distance])
        else:
            out.append(int(t))
    return bytes(out[len(prefix):])


def zlib_wrap(deflate, raw, header=b"\x78\x9c", adler=None):
    """A zlib stream around deflate bytes: header, data, the Adler-32 of `raw`."""
    return header + deflate + struct.pack(">I", zlib.adler32(raw) if adler is None else adler)


# ------------------------------------------------------------------ reading a block header
class _Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _canonical(lens):
    code, table = 0, {}
    for length in range(1, 16):
        for sym, l in enumerate(lens):
            if l == length:
                table[(length, code)] = sym
                code += 1
        code <<= 1
    return table


def first_block(deflate):
    """What the first block's header of a raw deflate stream says: {"final", "type"} and for a
    dynamic block also "nlen", "ndist", "lit_lens", "dist_lens", "cl_symbols" (the code-length
    symbols in the order they were read) and "crossing" (a repeat code filled lengths on both
    sides of the literal/length | distance boundary)."""
    b = _Bits(deflate)
    info = {"final": b.take(1), "type": b.take(2)}
    if info["type"] != 2:
        return info
    nlen, ndist, ncode = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    cl = [0] * 19
    for i in range(ncode):
        cl[CL_ORDER[i]] = b.take(3)
    table = _canonical(cl)
    lens, symbols, crossing = [], [], False
    while len(lens) < nlen + ndist:
        code, length = 0, 0
        while (length, code) not in table:
            code = code << 1 | b.take(1)
            length += 1
            assert length <= 7
        s = table[(length, code)]
        symbols.append(s)
        before = len(lens)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + b.take(2))
        elif s == 17:
            lens += [0] * (3 + b.take(3))
        else:
            lens += [0] * (11 + b.take(7))
        if s >= 16 and before < nlen < len(lens):
            crossing = True
    info.update(nlen=nlen, ndist=ndist, lit_lens=lens[:nlen], dist_lens=lens[nlen:nlen + ndist], cl_symbols=symbols,
                crossing=crossing)
    return info


# ------------------------------------------------------------------ damage
def flip_bit(data, byte, bit=0):
    out = bytearray(data)
    out[byte] ^= 1 << bit
    return bytes(out)


def flip_crc_bit(png):
    """The file with one bit of its first IDAT chunk's CRC flipped."""
    i = png.index(b"IDAT")
    (length,) = struct.unpack_from(">I", png, i - 4)
    return flip_bit(png, i + 4 + length)


def without_iend(png):
    assert png[-12:] == chunk(b"IEND")
    return png[:-12]
