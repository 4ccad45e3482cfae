// png.hip — 8-bit RGB PNG frames decoded on gfx950: the zlib stream of a file's IDAT chunks
// (without its 2-byte header) -> the tight (h, w, 3) image, every byte what Pillow's
// Image.open(path).convert("RGB") gives.  The host parses the chunks and checks their CRCs
// (monodepth2_amd/png_ops.py); the device does every per-byte job in two launches, and the
// launch boundary is what hands the first stage's bytes to the second:
//
//   inflate   one wave per stream (RFC 1951; stored, fixed and dynamic blocks).  Symbol
//             decoding is serial, so the wave decodes in lock step (every lane holds the same
//             bit buffer) and its lanes share the copies: a match is copied 64 bytes per
//             step, a stored block likewise.  The last 32768 output bytes live in an LDS ring,
//             so a match never reads global memory and nothing waits for a store to drain;
//             the ring is written out to the workspace 16 bytes per lane whenever 4 KiB have
//             gathered.  The compressed bytes come through a 2 KiB LDS buffer that is refilled
//             1 KiB at a time from a load issued one refill earlier.  A code is looked up in a
//             10-bit primary table in LDS; a longer one walks the canonical counts.
//   unfilter  one wave per image, one lane per row, 64 rows in flight: lane r is one pixel
//             behind lane r - 1, takes the pixel above from it with a cross-lane move and
//             keeps the pixels to the left and above-left in registers.  Bands of 64 rows
//             follow each other; the first row of a band reads the last row of the band
//             before from `out` behind a workgroup barrier.  The same pass sums the raw bytes
//             for the Adler-32 (per row: sum b and sum (len - j) b_j in 64 bits), combined in
//             row order mod 65521 and compared with the stream's last four bytes.
//
// Integer arithmetic only, no atomics: two runs are bit-equal.  Every write is bounded: the
// ring index is masked, an image's workspace range is align16(h (1 + 3 w)) bytes and the
// output position never passes h (1 + 3 w), so a corrupt stream writes nothing outside its own
// ranges and sets only its own status word.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

namespace {

constexpr int kMaxImages = 4096;   // per call
constexpr int kMaxDim = 8192;
constexpr int kWave = 64;
constexpr uint32_t kRing = 32768;            // the largest distance: byte p lives at ring[p & kRingMask]
constexpr uint32_t kRingMask = kRing - 1;
constexpr uint32_t kFlush = 4096;            // bytes gathered before the ring is written out
constexpr int kPrimaryBits = 10;
constexpr int kPrimary = 1 << kPrimaryBits;
constexpr uint32_t kChunkBytes = 16 * kWave;   // one refill of the input buffer: 16 bytes per lane
constexpr uint32_t kChunkWords = kChunkBytes / 4;
constexpr uint32_t kInWords = 2 * kChunkWords;

constexpr unsigned char kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__host__ __device__ inline uint64_t raw_bytes(int h, int w) { return (uint64_t)h * (1 + 3 * (uint64_t)w); }
__host__ __device__ inline uint64_t align16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

// Lanes of one wave hand bytes to each other through LDS.  The wave's LDS operations execute
// in order, so no instruction is needed; the fences keep the compiler from moving accesses.
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// Where image `img`'s range starts in the workspace: the sum of the ranges before it.
__device__ inline uint64_t workspace_offset(const md2_png_image* images, int img, int lane) {
    unsigned long long sum = 0;
    for (int i = lane; i < img; i += kWave) sum += align16(raw_bytes(images[i].height, images[i].width));
    for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    const uint32_t lo = uniform((uint32_t)sum), hi = uniform((uint32_t)(sum >> 32));
    return ((uint64_t)hi << 32) | lo;
}

struct Huff {
    uint16_t primary[kPrimary];   // symbol << 4 | length for a code of at most 10 bits, else 0
    uint16_t count[16];           // codes of each length
    uint16_t symbol[288];         // symbols ordered by (length, symbol)
};

// The compressed bytes of one stream, LSB first.  Every lane holds the same state.
struct Reader {
    const uint8_t* src;
    uint32_t nbytes;
    uint32_t* in;        // LDS, kInWords: chunk c lies in half c & 1
    uint64_t bb;
    uint32_t bc;         // valid bits in bb
    uint32_t inword;     // the next 32-bit word of the stream to enter bb
    uint4 pending;       // this lane's 16 bytes of the chunk after the two in LDS
    int lane;

    // Bytes past the stream's end read as zero; the decoder notices through overrun().
    __device__ __forceinline__ uint4 load(uint32_t chunk) const {
        const uint64_t off = (uint64_t)chunk * kChunkBytes + 16u * lane;
        if (off + 16 <= nbytes) return *reinterpret_cast<const uint4*>(src + off);
        uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t b = off + k < nbytes ? src[off + k] : 0u;
            if (k < 4) w0 |= b << (8 * (k & 3));
            else if (k < 8) w1 |= b << (8 * (k & 3));
            else if (k < 12) w2 |= b << (8 * (k & 3));
            else w3 |= b << (8 * (k & 3));
        }
        return make_uint4(w0, w1, w2, w3);
    }
    __device__ __forceinline__ void store(uint32_t half, uint4 v) {
        reinterpret_cast<uint4*>(in)[(half & 1) * kWave + lane] = v;
    }

    __device__ __forceinline__ void refill() {
        if (bc <= 32) {
            const uint32_t w = uniform(in[inword & (kInWords - 1)]);
            bb |= (uint64_t)w << bc;
            bc += 32;
            ++inword;
            if (inword % kChunkWords == 0) {   // chunk k is used up: k + 2 takes its half
                const uint32_t k = inword / kChunkWords - 1;
                wave_sync();
                store(k, pending);
                wave_sync();
                pending = load(k + 3);
            }
        }
    }
    __device__ void drop(uint32_t n) { bb >>= n; bc -= n; }
    __device__ uint32_t bits(uint32_t n) {   // n <= 16, after a refill
        const uint32_t v = (uint32_t)bb & ((1u << n) - 1);
        drop(n);
        return v;
    }
    __device__ uint64_t consumed() const { return (uint64_t)inword * 32 - bc; }
    __device__ bool overrun() const { return consumed() > (uint64_t)nbytes * 8; }
    // What a failed lookup means: with fewer than 15 bits of the stream left, the zeros behind
    // its end were part of the pattern, and zlib would have asked for more input.
    __device__ uint32_t no_code() const {
        return consumed() + 15 > (uint64_t)nbytes * 8 ? MD2_PNG_ST_END : MD2_PNG_ST_CODE;
    }
    __device__ __forceinline__ void seek(uint32_t byte) {
        const uint32_t c = byte / kChunkBytes;
        wave_sync();
        store(c, load(c));
        store(c + 1, load(c + 1));
        pending = load(c + 2);
        wave_sync();
        inword = byte >> 2;
        bb = 0;
        bc = 0;
        refill();
        drop(8 * (byte & 3));
    }
    __device__ __forceinline__ void seek_bit(uint64_t bit) {   // bit <= 8 * nbytes
        seek((uint32_t)(bit >> 3));
        drop((uint32_t)bit & 7);               // a seek leaves at least 8 bits
    }
};

// The tables of a set of code lengths, as zlib's inflate_table judges it: an over-subscribed
// set is refused, an incomplete one too unless it is a single code of one bit (code-length
// codes: always refused); no code at all is accepted and every lookup then fails.
__device__ int build(Huff& h, const uint8_t* lens, int n, bool code_lengths, uint16_t* codes, uint16_t* work,
                     int lane) {
    for (int i = lane; i < kPrimary; i += kWave) h.primary[i] = 0;
    uint32_t ok = 1;
    if (lane == 0) {
        for (int l = 0; l < 16; ++l) h.count[l] = 0;
        for (int s = 0; s < n; ++s) h.count[lens[s]]++;
        int left = 1, maxl = 0;
        for (int l = 1; l < 16; ++l) {
            left = 2 * left - h.count[l];
            if (left < 0) break;
            if (h.count[l]) maxl = l;
        }
        if (left < 0) ok = 0;
        else if (left > 0 && maxl != 0 && (code_lengths || maxl != 1)) ok = 0;
        if (ok) {
            uint32_t offs = 0, code = 0;
            work[0] = 0;
            work[16] = 0;
            for (int l = 1; l < 16; ++l) {
                work[l] = offs;                 // where the symbols of length l start
                offs += h.count[l];
                code = (code + (l > 1 ? h.count[l - 1] : 0)) << 1;
                work[16 + l] = code;            // the first code of length l
            }
            for (int s = 0; s < n; ++s) {
                const int l = lens[s];
                if (l) {
                    h.symbol[work[l]++] = s;
                    codes[s] = work[16 + l]++;
                }
            }
        }
    }
    wave_sync();
    ok = uniform(ok);
    if (!ok) return 0;
    for (int s = lane; s < n; s += kWave) {
        const uint32_t l = lens[s];
        if (l && l <= kPrimaryBits) {
            const uint32_t r = __brev((uint32_t)codes[s]) >> (32 - l);
            for (uint32_t k = r; k < kPrimary; k += 1u << l) h.primary[k] = (uint16_t)(s << 4 | l);
        }
    }
    wave_sync();
    return 1;
}

// One symbol, or -1 for a bit pattern that is no code.  Needs 15 bits in the buffer.
__device__ __forceinline__ int decode(const Huff& h, Reader& br) {
    const uint32_t e = uniform(h.primary[(uint32_t)br.bb & (kPrimary - 1)]);
    if (e) {
        br.drop(e & 15);
        return e >> 4;
    }
    int code = 0, first = 0, index = 0;
    uint32_t bits = (uint32_t)br.bb;
    for (int len = 1; len <= 15; ++len) {
        code |= bits & 1;
        bits >>= 1;
        const int cnt = uniform(h.count[len]);
        if (code - cnt < first) {
            br.drop(len);
            return uniform(h.symbol[index + (code - first)]);
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

// What the walk of a stream's blocks needs in LDS besides its window.
struct Scratch {
    Huff lit, dst;
    uint8_t lens[320];
    uint8_t cl_lens[19];
    uint16_t codes[320];
    uint16_t work[32];
};

// One entry of a stream's index (md2hot.h): where a segment of the output starts.
struct IndexEntry {
    unsigned long long header_bit;   // the 3-bit header of the block the segment starts in
    unsigned long long symbol_bit;   // the segment's first symbol (a stored block: its first byte)
    uint32_t out_pos;                // the output position the segment starts at
    uint32_t zero;
};
static_assert(sizeof(IndexEntry) == 24, "the index layout of md2hot.h");
constexpr uint32_t kIndexHeader = 16;   // u32 count, u32 segment_bytes, 8 zero bytes
constexpr uint32_t kMaxSymbol = 258;    // the most one symbol adds to the output

// The three uses of the one walk: kRun inflates into the 32 KiB byte ring and the workspace
// (md2_png_run); kIndex follows the same symbols, writes no byte and records where segments
// start; kSegment enters at an index entry and decodes one segment into 16-bit symbols.
enum Mode { kRun, kIndex, kSegment };

// kIndex: the entries found so far.  Every lane holds the same state; lane 0 writes.
struct Indexer {
    IndexEntry* entries;
    uint32_t cap, count, seg_start, segment_bytes;
    // a boundary candidate at output position pos: a new segment starts here if the current one is full
    __device__ void candidate(uint64_t header_bit, uint64_t symbol_bit, uint32_t pos, int lane) {
        if (pos - seg_start < segment_bytes) return;
        if (count < cap && lane == 0) {
            IndexEntry e;
            e.header_bit = header_bit;
            e.symbol_bit = symbol_bit;
            e.out_pos = pos;
            e.zero = 0;
            entries[count] = e;
        }
        ++count;
        seg_start = pos;
    }
};

// kSegment: the entry the wave starts from and where it stopped.
struct Segment {
    uint64_t header_bit, symbol_bit;
    uint32_t start, limit;   // the segment's output range
    uint32_t segment_bytes;  // S: a candidate at or past start + S inside the range is a boundary the index lacks
    bool last;               // the image's last segment: limit is the image's end
    uint64_t exit_header, exit_symbol;   // the candidate the wave stopped at (not for the last segment)
};

// The walk of one stream's blocks by one wave.  Returns the status bits of the inflate stage;
// `pos` is where the output stands afterwards.  window: kRun the byte ring (kRing bytes),
// kSegment the segment's symbols (uint16, position p at p - sg.start), kIndex unused.
template <int M>
__device__ __forceinline__ uint32_t inflate_walk(Reader& br, Scratch& sc, const uint32_t total, const int lane,
                                                 void* window, uint8_t* ws, Indexer& ix, Segment& sg, uint32_t& pos) {
    Huff& lit = sc.lit;
    Huff& dst = sc.dst;
    uint8_t* const lens = sc.lens;
    uint8_t* const cl_lens = sc.cl_lens;
    uint16_t* const codes = sc.codes;
    uint16_t* const work = sc.work;
    uint8_t* const ring = static_cast<uint8_t*>(window);
    uint16_t* const seg = static_cast<uint16_t*>(window);

    uint32_t flushed = 0, st = 0;
    uint32_t limit = total;      // where the output of this walk ends
    bool entering = false;       // kSegment: the first symbol is not the block's first
    bool stopped = false;        // kSegment: the walk reached its limit at a candidate
    pos = 0;
    if constexpr (M == kSegment) {
        pos = sg.start;
        limit = sg.limit;
        entering = sg.symbol_bit != sg.header_bit;
        br.seek_bit(sg.header_bit);
    } else {
        br.seek(0);
    }

    // the ring's bytes [flushed, upto) to the workspace; upto is a multiple of 16, at most align16(total)
    auto flush = [&](uint32_t upto) {
        wave_sync();
        for (uint32_t o = flushed + 16u * lane; o < upto; o += 16u * kWave)
            *reinterpret_cast<uint4*>(ws + o) = *reinterpret_cast<const uint4*>(ring + (o & kRingMask));
        flushed = upto;
    };

    while (true) {
        br.refill();
        [[maybe_unused]] const uint64_t header = br.consumed();   // a block header is a boundary candidate
        if constexpr (M == kIndex) ix.candidate(header, header, pos, lane);
        if constexpr (M == kSegment) {
            if (pos >= limit) {   // only a segment that is not the last comes here
                sg.exit_header = sg.exit_symbol = header;
                stopped = true;
                break;
            }
            if (pos - sg.start >= sg.segment_bytes) {   // a new segment starts at the FIRST such candidate
                st = MD2_PNG_ST_INDEX;
                break;
            }
        }
        const uint32_t last = br.bits(1), type = br.bits(2);
        if (type == 3) {
            st = MD2_PNG_ST_BLOCK;
            break;
        }
        if (type == 0) {
            br.drop(br.bc & 7);
            br.refill();
            uint32_t len = br.bits(16);
            br.refill();
            const uint32_t nlen = br.bits(16);
            if (br.overrun()) break;
            if ((len ^ 0xFFFFu) != nlen) {
                st = MD2_PNG_ST_BLOCK;
                break;
            }
            uint32_t byte = (uint32_t)(br.consumed() >> 3);
            if constexpr (M == kSegment) {
                if (entering) {   // the entry names a byte inside this block
                    entering = false;
                    const uint32_t first = (uint32_t)(sg.symbol_bit >> 3);   // symbol_bit <= 8 * nbytes
                    if ((sg.symbol_bit & 7) || first < byte || first - byte >= len) {
                        st = MD2_PNG_ST_INDEX;
                        break;
                    }
                    len -= first - byte;
                    byte = first;
                }
            }
            if (len) {
                const uint32_t have = br.nbytes - byte;            // no overrun: byte <= nbytes
                uint32_t n = len < have ? len : have;
                if (n > limit - pos) n = limit - pos;
                const uint32_t end = byte + len;
                if constexpr (M == kSegment) {   // every byte is a candidate: the last one copied too
                    if (n && pos + n - 1 - sg.start >= sg.segment_bytes) {
                        st = MD2_PNG_ST_INDEX;
                        break;
                    }
                }
                if constexpr (M == kIndex) {   // every byte of the block is a candidate
                    uint32_t done = 0;
                    while (done < n) {
                        const uint32_t made = pos + done - ix.seg_start;
                        if (made >= ix.segment_bytes) {
                            ix.candidate(header, 8ull * (byte + done), pos + done, lane);
                            continue;
                        }
                        const uint32_t step = ix.segment_bytes - made;
                        done += step < n - done ? step : n - done;
                    }
                    pos += n;
                    byte += n;
                } else {
                    while (n) {
                        const uint32_t piece = n < kFlush ? n : kFlush;
                        wave_sync();
                        if constexpr (M == kRun) {
                            for (uint32_t i = lane; i < piece; i += kWave)
                                ring[(pos + i) & kRingMask] = br.src[byte + i];
                        } else {
                            for (uint32_t i = lane; i < piece; i += kWave) seg[pos - sg.start + i] = br.src[byte + i];
                        }
                        pos += piece;
                        byte += piece;
                        n -= piece;
                        if constexpr (M == kRun)
                            if (pos - flushed >= kFlush) flush(pos & ~15u);
                    }
                }
                if constexpr (M == kSegment) {
                    if (pos >= limit && !sg.last && byte < end) {   // the next byte of the block is the candidate
                        sg.exit_header = header;
                        sg.exit_symbol = 8ull * byte;
                        stopped = true;
                        break;
                    }
                    if (pos >= limit && sg.last) break;
                } else {
                    if (pos >= total) break;
                }
                if (len > have) {
                    st = MD2_PNG_ST_END;
                    break;
                }
                br.seek(end);
            }
        } else {
            if (type == 1) {
                for (int s = lane; s < 320; s += kWave)
                    lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
                wave_sync();
                build(lit, lens, 288, false, codes, work, lane);
                build(dst, lens + 288, 32, false, codes, work, lane);
            } else {
                br.refill();
                const uint32_t nl = br.bits(5) + 257, nd = br.bits(5) + 1, nc = br.bits(4) + 4;
                if (nl > 286 || nd > 30) {
                    st = MD2_PNG_ST_CODE;
                    break;
                }
                for (uint32_t i = 0; i < 19; ++i) {
                    br.refill();
                    const uint32_t v = i < nc ? br.bits(3) : 0;
                    if (lane == 0) cl_lens[kOrder[i]] = (uint8_t)v;
                }
                wave_sync();
                if (!build(dst, cl_lens, 19, true, codes, work, lane)) {
                    st = MD2_PNG_ST_CODE;
                    break;
                }
                uint32_t idx = 0, prev = 0, has_end = 0;
                const uint32_t nsym = nl + nd;
                while (idx < nsym) {
                    br.refill();
                    const int s = decode(dst, br);
                    uint32_t rep = 1, val = (uint32_t)s;
                    if (s < 0) {
                        st = br.no_code();
                        break;
                    }
                    if (s == 16) {
                        if (idx == 0) {
                            st = MD2_PNG_ST_CODE;
                            break;
                        }
                        rep = 3 + br.bits(2);
                        val = prev;
                    } else if (s == 17) {
                        rep = 3 + br.bits(3);
                        val = 0;
                    } else if (s == 18) {
                        rep = 11 + br.bits(7);
                        val = 0;
                    }
                    if (idx + rep > nsym) {
                        st = MD2_PNG_ST_CODE;
                        break;
                    }
                    if (idx <= 256 && 256 < idx + rep) has_end = val != 0;
                    if (lane == 0)
                        for (uint32_t k = 0; k < rep; ++k) lens[idx + k] = (uint8_t)val;
                    idx += rep;
                    prev = val;
                }
                if (!st && !has_end) st = MD2_PNG_ST_CODE;   // no end-of-block code
                if (st) break;
                wave_sync();
                if (!build(lit, lens, nl, false, codes, work, lane) ||
                    !build(dst, lens + nl, nd, false, codes, work, lane)) {
                    st = MD2_PNG_ST_CODE;
                    break;
                }
            }
            if constexpr (M == kSegment) {
                if (entering) {   // the entry names a symbol behind the block's tables
                    entering = false;
                    if (sg.symbol_bit < br.consumed()) {
                        st = MD2_PNG_ST_INDEX;
                        break;
                    }
                    br.seek_bit(sg.symbol_bit);
                }
            }
            while (true) {
                br.refill();
                if constexpr (M == kIndex) ix.candidate(header, br.consumed(), pos, lane);   // a symbol's start
                if constexpr (M == kSegment) {
                    if (pos - sg.start >= sg.segment_bytes) {
                        st = MD2_PNG_ST_INDEX;
                        break;
                    }
                }
                int sym = decode(lit, br);
                if (sym < 0) {
                    st = br.no_code();
                    break;
                }
                if (sym < 256) {
                    if constexpr (M == kRun) {
                        if (lane == 0) ring[pos & kRingMask] = (uint8_t)sym;
                    } else if constexpr (M == kSegment) {
                        if (lane == 0) seg[pos - sg.start] = (uint16_t)sym;
                    }
                    ++pos;
                } else if (sym == 256) {
                    break;
                } else {
                    if (sym > 285) {
                        st = MD2_PNG_ST_CODE;
                        break;
                    }
                    sym -= 257;
                    uint32_t len;
                    if (sym < 8) len = 3 + sym;
                    else if (sym == 28) len = 258;
                    else {
                        const uint32_t e = (sym >> 2) - 1;
                        len = 3 + ((4u + (sym & 3)) << e) + br.bits(e);
                    }
                    br.refill();
                    const int d = decode(dst, br);
                    if (d < 0 || d > 29) {
                        st = d < 0 ? br.no_code() : MD2_PNG_ST_CODE;
                        break;
                    }
                    uint32_t dist;
                    if (d < 4) dist = 1 + d;
                    else {
                        const uint32_t e = (d >> 1) - 1;
                        dist = 1 + ((2u + (d & 1)) << e) + br.bits(e);
                    }
                    if (br.overrun()) break;
                    if (dist > pos) {
                        st = MD2_PNG_ST_DIST;
                        break;
                    }
                    if (len > limit - pos) {
                        len = limit - pos;
                        if constexpr (M == kSegment)
                            if (!sg.last) st = MD2_PNG_ST_INDEX;   // a true entry lies between two symbols
                    }
                    const uint32_t from = pos - dist;
                    if constexpr (M == kRun) {
                        wave_sync();
                        if (dist >= len) {
                            for (uint32_t i = lane; i < len; i += kWave)
                                ring[(pos + i) & kRingMask] = ring[(from + i) & kRingMask];
                        } else {   // the copy repeats a period: byte i is source byte i mod dist
                            for (uint32_t i = lane; i < len; i += kWave)
                                ring[(pos + i) & kRingMask] = ring[(from + i % dist) & kRingMask];
                        }
                        wave_sync();
                    } else if constexpr (M == kSegment) {
                        // a source inside the segment is copied as the symbol it is (a marker stays a
                        // marker); one before it becomes 0x8000 | k: the byte k + 1 before the start
                        wave_sync();
                        for (uint32_t i = lane; i < len; i += kWave) {
                            const uint32_t q = from + (dist >= len ? i : i % dist);
                            seg[pos - sg.start + i] =
                                q >= sg.start ? seg[q - sg.start] : (uint16_t)(0x8000u | (sg.start - 1 - q));
                        }
                        wave_sync();
                    }
                    pos += len;
                    if constexpr (M == kSegment)
                        if (st) break;
                }
                if constexpr (M == kSegment) {
                    if (pos >= limit && !sg.last && !br.overrun()) {   // the next symbol's start is the candidate
                        sg.exit_header = header;
                        sg.exit_symbol = br.consumed();
                        stopped = true;
                        break;
                    }
                }
                if (pos >= limit || br.overrun()) break;
                if constexpr (M == kRun)
                    if (pos - flushed >= kFlush) flush(pos & ~15u);
            }
            if (st) break;
            if constexpr (M == kSegment)
                if (stopped) break;
        }
        if constexpr (M == kSegment) {   // a block that ends at the limit: the next header is the candidate
            if ((pos >= limit && sg.last) || br.overrun()) break;
        } else {
            if (pos >= limit || br.overrun()) break;
        }
        if (last) {
            st = MD2_PNG_ST_END;   // the last block ends before the image is complete
            break;
        }
        if constexpr (M == kRun)
            if (pos - flushed >= kFlush) flush(pos & ~15u);
    }
    if (br.overrun()) st = MD2_PNG_ST_END;   // whatever the zeros past the end decoded to
    if constexpr (M == kRun) flush((uint32_t)align16(pos));
    if constexpr (M == kSegment)
        if (!st && !sg.last && !stopped) st = MD2_PNG_ST_INDEX;
    return st;
}

__global__ __launch_bounds__(kWave) void png_inflate_kernel(const uint8_t* __restrict__ streams,
                                                            const md2_png_image* __restrict__ images,
                                                            uint8_t* __restrict__ workspace,
                                                            uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
    __shared__ __attribute__((aligned(16))) uint32_t in[kInWords];
    __shared__ Scratch sc;

    const int img = blockIdx.x, lane = threadIdx.x;
    const md2_png_image im = images[img];
    const uint32_t total = (uint32_t)raw_bytes(im.height, im.width);
    uint8_t* ws = workspace + workspace_offset(images, img, lane);

    Reader br;
    br.src = streams + im.stream_offset;
    br.nbytes = im.stream_bytes;
    br.in = in;
    br.lane = lane;
    Indexer ix{};
    Segment sg{};
    uint32_t pos;
    const uint32_t st = inflate_walk<kRun>(br, sc, total, lane, ring, ws, ix, sg, pos);
    if (lane == 0) status[img] = st;
}

// ---------------------------------------------------------------------------------------------
// The indexed decoder (md2hot.h): the output of a stream is cut into segments of at least
// segment_bytes bytes at boundary candidates; md2_png_index finds the cuts once with the serial
// walk, md2_png_run_indexed then decodes every segment of every image at the same time.

__host__ __device__ inline uint32_t seg_capacity(uint64_t raw, uint32_t segment_bytes) {
    return (uint32_t)(raw / segment_bytes) + 1;
}
__host__ __device__ inline uint64_t index_size(uint64_t raw, uint32_t segment_bytes) {
    return align16(kIndexHeader + (uint64_t)sizeof(IndexEntry) * seg_capacity(raw, segment_bytes));
}

// Where image `img`'s status words start among the per-segment words: the capacities before it.
__device__ inline uint32_t capacity_offset(const md2_png_image* images, int img, uint32_t segment_bytes, int lane) {
    uint32_t sum = 0;
    for (int i = lane; i < img; i += kWave)
        sum += seg_capacity(raw_bytes(images[i].height, images[i].width), segment_bytes);
    for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    return uniform(sum);
}

__global__ __launch_bounds__(kWave) void png_index_kernel(const uint8_t* __restrict__ streams,
                                                          const md2_png_image* __restrict__ images,
                                                          uint32_t segment_bytes, uint8_t* __restrict__ index,
                                                          const uint64_t* __restrict__ index_offsets,
                                                          uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint32_t in[kInWords];
    __shared__ Scratch sc;

    const int img = blockIdx.x, lane = threadIdx.x;
    const md2_png_image im = images[img];
    const uint32_t total = (uint32_t)raw_bytes(im.height, im.width);
    uint8_t* base = index + index_offsets[img];

    Reader br;
    br.src = streams + im.stream_offset;
    br.nbytes = im.stream_bytes;
    br.in = in;
    br.lane = lane;
    Indexer ix;
    ix.entries = reinterpret_cast<IndexEntry*>(base + kIndexHeader);
    ix.cap = seg_capacity(total, segment_bytes);
    ix.count = 1;   // segment 0: bit 0, output 0
    ix.seg_start = 0;
    ix.segment_bytes = segment_bytes;
    if (lane == 0) {
        IndexEntry e = {0, 0, 0, 0};
        ix.entries[0] = e;
    }
    Segment sg{};
    uint32_t pos;
    const uint32_t st = inflate_walk<kIndex>(br, sc, total, lane, nullptr, nullptr, ix, sg, pos);
    // a stream that did not inflate gets an index nothing can be decoded from: count 0
    const uint32_t count = (st || ix.count > ix.cap) ? 0 : ix.count;
    if (lane == 0) {
        uint32_t* head = reinterpret_cast<uint32_t*>(base);
        head[0] = count;
        head[1] = segment_bytes;
        head[2] = head[3] = 0;
        status[img] = st;
    }
    const uint32_t end = (uint32_t)index_size(total, segment_bytes);
    for (uint32_t o = kIndexHeader + (uint32_t)sizeof(IndexEntry) * count + 4u * lane; o < end; o += 4u * kWave)
        *reinterpret_cast<uint32_t*>(base + o) = 0;
}

// One wave per (image, segment).  Writes the segment's symbols at symbols[p] for the positions p
// of its own range [out_pos, next out_pos) and nothing else but its own status word.
template <int S>
__global__ __launch_bounds__(kWave) void png_segment_kernel(const uint8_t* __restrict__ streams,
                                                            const md2_png_image* __restrict__ images,
                                                            const uint64_t* __restrict__ index_offsets,
                                                            uint16_t* __restrict__ symbols,
                                                            uint32_t* __restrict__ seg_status) {
    __shared__ __attribute__((aligned(16))) uint16_t seg[S + kMaxSymbol + 6];   // S + 257 positions are enough
    __shared__ __attribute__((aligned(16))) uint32_t in[kInWords];
    __shared__ Scratch sc;

    const int img = blockIdx.y, lane = threadIdx.x;
    const uint32_t s = blockIdx.x;
    const md2_png_image im = images[img];
    const uint32_t total = (uint32_t)raw_bytes(im.height, im.width);
    const uint32_t cap = seg_capacity(total, S);
    if (s >= cap) return;   // the grid is as wide as the batch's largest image
    uint32_t* word = seg_status + capacity_offset(images, img, S, lane) + s;
    const uint8_t* ix = streams + index_offsets[img];
    const uint32_t count = reinterpret_cast<const uint32_t*>(ix)[0];
    const uint32_t stored_s = reinterpret_cast<const uint32_t*>(ix)[1];
    if (count < 1 || count > cap || stored_s != (uint32_t)S) {   // segment 0 speaks for the image
        if (lane == 0) *word = s == 0 ? MD2_PNG_ST_INDEX : 0;
        return;
    }
    if (s >= count) {
        if (lane == 0) *word = 0;
        return;
    }
    const IndexEntry* entries = reinterpret_cast<const IndexEntry*>(ix + kIndexHeader);
    const IndexEntry e = entries[s];
    IndexEntry next = e;
    Segment sg;
    sg.last = s == count - 1;
    if (!sg.last) next = entries[s + 1];
    sg.header_bit = e.header_bit;
    sg.symbol_bit = e.symbol_bit;
    sg.start = e.out_pos;
    sg.limit = sg.last ? total : next.out_pos;
    sg.segment_bytes = S;
    sg.exit_header = sg.exit_symbol = 0;

    uint32_t st = 0, pos = 0;
    if (e.header_bit > e.symbol_bit || e.symbol_bit > 8ull * im.stream_bytes || (s == 0 && (e.out_pos | e.header_bit | e.symbol_bit) != 0) ||
        sg.start >= sg.limit || sg.limit > total || sg.limit - sg.start > (uint32_t)S + kMaxSymbol - 1)
        st = MD2_PNG_ST_INDEX;
    if (!st) {
        Reader br;
        br.src = streams + im.stream_offset;
        br.nbytes = im.stream_bytes;
        br.in = in;
        br.lane = lane;
        Indexer none{};
        st = inflate_walk<kSegment>(br, sc, total, lane, seg, nullptr, none, sg, pos);
        if (!st && (pos != sg.limit || (!sg.last && (sg.exit_header != next.header_bit ||
                                                     sg.exit_symbol != next.symbol_bit))))
            st = MD2_PNG_ST_INDEX;
    }
    if (!st) {
        wave_sync();
        uint16_t* dstp = symbols + workspace_offset(images, img, lane) + sg.start;
        const uint32_t n = sg.limit - sg.start;
        for (uint32_t i = lane; i < n; i += kWave) dstp[i] = seg[i];
    }
    if (lane == 0) *word = st;
}

constexpr int kResolveThreads = 256;

// One workgroup per image: ORs the image's segment words into its status word and, if that is
// 0, turns the symbols into the scanline bytes segment after segment.  A marker of segment j
// reads a byte before the segment's start, which an earlier round of this workgroup wrote.
__global__ __launch_bounds__(kResolveThreads) void png_resolve_kernel(const uint8_t* __restrict__ streams,
                                                                      const md2_png_image* __restrict__ images,
                                                                      const uint64_t* __restrict__ index_offsets,
                                                                      uint32_t segment_bytes, uint8_t* workspace,
                                                                      const uint16_t* __restrict__ symbols,
                                                                      const uint32_t* __restrict__ seg_status,
                                                                      uint32_t* __restrict__ status) {
    __shared__ uint32_t bits;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1);
    const md2_png_image im = images[img];
    const uint32_t total = (uint32_t)raw_bytes(im.height, im.width);
    const uint32_t cap = seg_capacity(total, segment_bytes);
    const uint32_t* words = seg_status + capacity_offset(images, img, segment_bytes, lane);
    uint32_t mine = 0;
    for (uint32_t j = tid; j < cap; j += kResolveThreads) mine |= words[j];
    if (tid == 0) bits = 0;
    __syncthreads();
    if (mine) atomicOr(&bits, mine);   // an integer OR in LDS: the order does not matter
    __syncthreads();
    const uint32_t st = bits;
    if (tid == 0) status[img] = st;
    if (st) return;   // the scanlines are not complete: nothing is resolved, nothing unfiltered

    // every segment wave found its entry and the next consistent: the entries cover [0, total)
    const uint64_t off = workspace_offset(images, img, lane);
    uint8_t* ws = workspace + off;
    const uint16_t* sym = symbols + off;
    const uint8_t* ix = streams + index_offsets[img];
    const uint32_t count = reinterpret_cast<const uint32_t*>(ix)[0];
    const IndexEntry* entries = reinterpret_cast<const IndexEntry*>(ix + kIndexHeader);
    uint32_t start = 0;
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t end = j + 1 < count ? entries[j + 1].out_pos : total;
        for (uint32_t p = start + tid; p < end; p += kResolveThreads) {
            const uint32_t v = sym[p];
            ws[p] = (v & 0x8000u) ? ws[start - 1 - (v & 0x7FFFu)] : (uint8_t)v;
        }
        // segment j is final before segment j + 1 reads it: the workgroup's own writes, made
        // visible to the workgroup, behind the workgroup's own barrier
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        start = end;
    }
}

__device__ inline int paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ inline uint32_t unfilter(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t p = 0;
    if (ft == 1) p = a;
    else if (ft == 2) p = b;
    else if (ft == 3) p = (a + b) >> 1;
    else if (ft == 4) p = (uint32_t)paeth((int)a, (int)b, (int)c);
    return (x + p) & 255u;
}

__global__ __launch_bounds__(kWave) void png_unfilter_kernel(const uint8_t* __restrict__ streams,
                                                             const md2_png_image* __restrict__ images,
                                                             const uint8_t* __restrict__ workspace,
                                                             uint8_t* out, uint32_t* status) {
    __shared__ uint32_t row_s1[kWave];
    __shared__ unsigned long long row_s2[kWave];
    const int img = blockIdx.x, lane = threadIdx.x;
    if (status[img] != 0) return;   // the scanlines are not complete
    const md2_png_image im = images[img];
    const int h = im.height, w = im.width;
    const uint32_t len = 1 + 3 * (uint32_t)w;
    const uint8_t* raw = workspace + workspace_offset(images, img, lane);
    uint8_t* dst = out + im.out_offset;
    uint32_t adler_a = 1, adler_b = 0, bad_filter = 0;

    for (int r0 = 0; r0 < h; r0 += kWave) {
        if (r0) __syncthreads();   // the band before has stored its last row
        const int r = r0 + lane;
        const bool active = r < h;
        const uint8_t* rp = raw + (uint64_t)(active ? r : 0) * len;
        uint8_t* op = dst + (uint64_t)(active ? r : 0) * 3 * w;
        const uint8_t* up = dst + (uint64_t)(r0 ? r0 - 1 : 0) * 3 * w;
        const uint32_t ft_raw = active ? rp[0] : 0;
        uint32_t ft = ft_raw;
        if (ft > 4) {
            bad_filter = 1;
            ft = 0;
        }
        uint32_t s1 = ft_raw;
        unsigned long long s2 = (unsigned long long)len * ft_raw;
        uint32_t a = 0, c = 0, cur = 0;   // packed R | G << 8 | B << 16: left, above-left, this lane's last pixel
        uint32_t n0 = 0, n1 = 0, n2 = 0;  // the raw bytes of the next pixel
        if (active && lane == 0) {
            n0 = rp[1];
            n1 = rp[2];
            n2 = rp[3];
        }
        for (int t = 0; t < w + kWave - 1; ++t) {
            const int x = t - lane;
            uint32_t b = __shfl_up(cur, 1);
            const bool v = active && x >= 0 && x < w;
            if (lane == 0) {
                b = 0;
                if (v && r0) b = up[3 * x] | (uint32_t)up[3 * x + 1] << 8 | (uint32_t)up[3 * x + 2] << 16;
            }
            const uint32_t x0 = n0, x1 = n1, x2 = n2;
            if (active && x + 1 >= 0 && x + 1 < w) {
                n0 = rp[4 + 3 * x];
                n1 = rp[5 + 3 * x];
                n2 = rp[6 + 3 * x];
            }
            if (v) {
                const uint32_t o0 = unfilter(ft, x0, a & 255, b & 255, c & 255);
                const uint32_t o1 = unfilter(ft, x1, (a >> 8) & 255, (b >> 8) & 255, (c >> 8) & 255);
                const uint32_t o2 = unfilter(ft, x2, a >> 16, b >> 16, c >> 16);
                op[3 * x] = (uint8_t)o0;
                op[3 * x + 1] = (uint8_t)o1;
                op[3 * x + 2] = (uint8_t)o2;
                s1 += x0 + x1 + x2;
                const uint32_t wgt = len - 1 - 3 * (uint32_t)x;   // the weight of the pixel's first byte
                s2 += (unsigned long long)wgt * x0 + (unsigned long long)(wgt - 1) * x1 +
                      (unsigned long long)(wgt - 2) * x2;
                c = b;
                a = cur = o0 | o1 << 8 | o2 << 16;
            }
        }
        row_s1[lane] = s1;
        row_s2[lane] = s2;
        __syncthreads();
        if (lane == 0) {
            const int rows = h - r0 < kWave ? h - r0 : kWave;
            for (int i = 0; i < rows; ++i) {
                adler_b = (uint32_t)((adler_b + (unsigned long long)len * adler_a + row_s2[i] % 65521u) % 65521u);
                adler_a = (adler_a + row_s1[i] % 65521u) % 65521u;
            }
        }
        __syncthreads();
    }
    const bool any_bad = __any(bad_filter) != 0;
    if (lane == 0) {
        uint32_t st = any_bad ? MD2_PNG_ST_FILTER : 0;
        const uint8_t* s = streams + im.stream_offset;
        const uint32_t nb = im.stream_bytes;
        uint32_t trailer = 0;
        if (nb >= 4)
            trailer = (uint32_t)s[nb - 4] << 24 | (uint32_t)s[nb - 3] << 16 | (uint32_t)s[nb - 2] << 8 | s[nb - 1];
        if (nb < 4 || trailer != (adler_b << 16 | adler_a)) st |= MD2_PNG_ST_ADLER;
        if (st) status[img] = st;
    }
}

const char* check_images(const md2_png_image* images, int n) {
    if (n < 0 || n > kMaxImages) return "png: n must be 0..4096";
    if (n && !images) return "png: images is NULL";
    for (int i = 0; i < n; ++i)
        if (images[i].height < 1 || images[i].height > kMaxDim || images[i].width < 1 || images[i].width > kMaxDim)
            return "png: height and width must be 1..8192";
    return nullptr;
}

const char* check_ranges(const md2_png_image* images, int n, uint64_t streams_bytes, uint64_t out_bytes,
                         bool with_out = true) {
    for (int i = 0; i < n; ++i) {
        const md2_png_image& im = images[i];
        if (im.stream_offset % 16 || (with_out && im.out_offset % 16))
            return "png: stream_offset and out_offset must be multiples of 16";
        if (im.stream_offset > streams_bytes || im.stream_bytes > streams_bytes - im.stream_offset)
            return "png: a stream reaches past streams_bytes";
        if (!with_out) continue;
        const uint64_t ob = (uint64_t)im.height * im.width * 3;
        if (im.out_offset > out_bytes || ob > out_bytes - im.out_offset) return "png: a frame reaches past out_bytes";
    }
    return nullptr;
}

size_t workspace_need(const md2_png_image* images, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += align16(raw_bytes(images[i].height, images[i].width));
    return total;
}

const char* check_segment_bytes(int segment_bytes) {
    if (segment_bytes < 1024 || segment_bytes > 32768 || (segment_bytes & (segment_bytes - 1)))
        return "png: segment_bytes must be a power of two in 1024..32768";
    return nullptr;
}

// every image's index lies, 16-byte aligned, inside a buffer of `bytes` bytes (`past`: what to say if not)
const char* check_index(const md2_png_image* images, const uint64_t* index_offsets, int n, int segment_bytes,
                        uint64_t bytes, const char* past) {
    for (int i = 0; i < n; ++i) {
        if (index_offsets[i] % 16) return "png: an index offset must be a multiple of 16";
        const uint64_t ib = index_size(raw_bytes(images[i].height, images[i].width), segment_bytes);
        if (index_offsets[i] > bytes || ib > bytes - index_offsets[i]) return past;
    }
    return nullptr;
}

size_t indexed_workspace_need(const md2_png_image* images, int n, int segment_bytes) {
    uint64_t words = 0;
    for (int i = 0; i < n; ++i) words += seg_capacity(raw_bytes(images[i].height, images[i].width), segment_bytes);
    return 3 * workspace_need(images, n) + align16(4 * words);
}

template <int S>
void launch_segments(dim3 grid, hipStream_t st, const uint8_t* streams, const md2_png_image* dev_images,
                     const uint64_t* dev_index_offsets, uint16_t* symbols, uint32_t* seg_status) {
    hipLaunchKernelGGL(png_segment_kernel<S>, grid, dim3(kWave), 0, st, streams, dev_images, dev_index_offsets, symbols,
                       seg_status);
}

}  // namespace

extern "C" {

size_t md2_png_index_bytes(int height, int width, int segment_bytes) {
    const char* msg = check_segment_bytes(segment_bytes);
    if (!msg && (height < 1 || height > kMaxDim || width < 1 || width > kMaxDim))
        msg = "png: height and width must be 1..8192";
    if (msg) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return index_size(raw_bytes(height, width), segment_bytes);
}

size_t md2_png_indexed_workspace_bytes(const md2_png_image* images, int n, int segment_bytes) {
    const char* msg = check_images(images, n);
    if (!msg) msg = check_segment_bytes(segment_bytes);
    if (msg) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return indexed_workspace_need(images, n, segment_bytes);
}

int md2_png_index(const uint8_t* streams, uint64_t streams_bytes, const md2_png_image* images,
                  const md2_png_image* dev_images, int n, int segment_bytes, uint8_t* index, uint64_t index_bytes,
                  const uint64_t* index_offsets, const uint64_t* dev_index_offsets, uint32_t* status, void* stream) {
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_segment_bytes(segment_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    if (n == 0) return MD2_OK;
    if (!streams || !dev_images || !index || !index_offsets || !dev_index_offsets || !status)
        return md2_report_error(MD2_ERR_ARG,
                                "png: streams/dev_images/index/index_offsets/dev_index_offsets/status is NULL");
    if (const char* msg = check_ranges(images, n, streams_bytes, ~(uint64_t)0, false))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_index(images, index_offsets, n, segment_bytes, index_bytes,
                                      "png: an index reaches past index_bytes"))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (reinterpret_cast<uintptr_t>(streams) % 16 || reinterpret_cast<uintptr_t>(index) % 16 ||
        reinterpret_cast<uintptr_t>(dev_images) % 8 || reinterpret_cast<uintptr_t>(dev_index_offsets) % 8)
        return md2_report_error(MD2_ERR_ARG,
                                "png: streams and index must be 16-byte, dev_images and dev_index_offsets 8-byte aligned");
    hipLaunchKernelGGL(png_index_kernel, dim3(n), dim3(kWave), 0, (hipStream_t)stream, streams, dev_images,
                       (uint32_t)segment_bytes, index, dev_index_offsets, status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

int md2_png_check_indexed(const md2_png_image* images, const uint64_t* index_offsets, int n, int segment_bytes,
                          uint64_t streams_bytes, uint64_t out_bytes) {
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_segment_bytes(segment_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    if (n && !index_offsets) return md2_report_error(MD2_ERR_ARG, "png: index_offsets is NULL");
    if (const char* msg = check_ranges(images, n, streams_bytes, out_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_index(images, index_offsets, n, segment_bytes, streams_bytes,
                                      "png: an index reaches past streams_bytes"))
        return md2_report_error(MD2_ERR_ARG, msg);
    return MD2_OK;
}

int md2_png_run_indexed(const uint8_t* streams, uint64_t streams_bytes, const md2_png_image* images,
                        const md2_png_image* dev_images, const uint64_t* index_offsets,
                        const uint64_t* dev_index_offsets, int n, int segment_bytes, uint8_t* workspace,
                        size_t workspace_bytes, uint8_t* out, uint64_t out_bytes, uint32_t* status, void* stream) {
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_segment_bytes(segment_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    if (n == 0) return MD2_OK;
    if (!streams || !dev_images || !index_offsets || !dev_index_offsets || !workspace || !out || !status)
        return md2_report_error(
            MD2_ERR_ARG, "png: streams/dev_images/index_offsets/dev_index_offsets/workspace/out/status is NULL");
    if (const char* msg = check_ranges(images, n, streams_bytes, out_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_index(images, index_offsets, n, segment_bytes, streams_bytes,
                                      "png: an index reaches past streams_bytes"))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (reinterpret_cast<uintptr_t>(streams) % 16 || reinterpret_cast<uintptr_t>(workspace) % 16 ||
        reinterpret_cast<uintptr_t>(dev_images) % 8 || reinterpret_cast<uintptr_t>(dev_index_offsets) % 8)
        return md2_report_error(
            MD2_ERR_ARG,
            "png: streams and workspace must be 16-byte, dev_images and dev_index_offsets 8-byte aligned");
    if (indexed_workspace_need(images, n, segment_bytes) > workspace_bytes)
        return md2_report_error(MD2_ERR_ARG, "png: the batch needs more workspace than workspace_bytes");
    const size_t scan = workspace_need(images, n);
    uint16_t* symbols = reinterpret_cast<uint16_t*>(workspace + scan);
    uint32_t* seg_status = reinterpret_cast<uint32_t*>(workspace + 3 * scan);
    uint32_t widest = 1;
    for (int i = 0; i < n; ++i) {
        const uint32_t c = seg_capacity(raw_bytes(images[i].height, images[i].width), segment_bytes);
        widest = c > widest ? c : widest;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(widest, n);
    switch (segment_bytes) {
        case 1024: launch_segments<1024>(grid, st, streams, dev_images, dev_index_offsets, symbols, seg_status); break;
        case 2048: launch_segments<2048>(grid, st, streams, dev_images, dev_index_offsets, symbols, seg_status); break;
        case 4096: launch_segments<4096>(grid, st, streams, dev_images, dev_index_offsets, symbols, seg_status); break;
        case 8192: launch_segments<8192>(grid, st, streams, dev_images, dev_index_offsets, symbols, seg_status); break;
        case 16384: launch_segments<16384>(grid, st, streams, dev_images, dev_index_offsets, symbols, seg_status); break;
        default: launch_segments<32768>(grid, st, streams, dev_images, dev_index_offsets, symbols, seg_status); break;
    }
    hipLaunchKernelGGL(png_resolve_kernel, dim3(n), dim3(kResolveThreads), 0, st, streams, dev_images,
                       dev_index_offsets, (uint32_t)segment_bytes, workspace, symbols, seg_status, status);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(kWave), 0, st, streams, dev_images, workspace, out, status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

size_t md2_png_workspace_bytes(const md2_png_image* images, int n) {
    if (const char* msg = check_images(images, n)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return workspace_need(images, n);
}

int md2_png_check(const md2_png_image* images, int n, uint64_t streams_bytes, uint64_t out_bytes) {
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, streams_bytes, out_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    return MD2_OK;
}

int md2_png_run(const uint8_t* streams, uint64_t streams_bytes, const md2_png_image* images,
                const md2_png_image* dev_images, int n, uint8_t* workspace, size_t workspace_bytes, uint8_t* out,
                uint64_t out_bytes, uint32_t* status, void* stream) {
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (n == 0) return MD2_OK;
    if (!streams || !dev_images || !workspace || !out || !status)
        return md2_report_error(MD2_ERR_ARG, "png: streams/dev_images/workspace/out/status is NULL");
    if (const char* msg = check_ranges(images, n, streams_bytes, out_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    if (reinterpret_cast<uintptr_t>(streams) % 16 || reinterpret_cast<uintptr_t>(workspace) % 16 ||
        reinterpret_cast<uintptr_t>(dev_images) % 8)
        return md2_report_error(MD2_ERR_ARG, "png: streams and workspace must be 16-byte, dev_images 8-byte aligned");
    if (workspace_need(images, n) > workspace_bytes)
        return md2_report_error(MD2_ERR_ARG, "png: the batch needs more workspace than workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(kWave), 0, st, streams, dev_images, workspace, status);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(kWave), 0, st, streams, dev_images, workspace, out, status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
