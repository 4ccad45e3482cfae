// pngenc.hip — PNG encoding on gfx950: the other half of png.hip.  Tight (h, w, 3) uint8 RGB
// frames and (h, w) 16-bit grey maps of mixed sizes -> the zlib stream of each file's IDAT
// chunk (the host writes the chunks and their CRCs, monodepth2_amd/png_ops.py).  The format
// rules are DESIGN.md §6n; tests/png_encode_case.py restates them and the output is held to
// that restatement byte for byte.  Three launches, and the launch boundaries hand the bytes on:
//
//   filter    one wave per row: the five filters' sums of |signed residual| over the row, the
//             least one (ties to the lowest number) written to the workspace behind its filter
//             byte, and the row's two Adler-32 sums (sum b, sum (len - j) b_j).
//   deflate   one wave per segment of S filtered bytes, all segments of all images at once.  A
//             step takes 64 positions, one per lane: each looks up its candidates (distance 1,
//             and the hash table's entry as the step before left it), then all insert; the
//             greedy parse of the step runs on the wave-uniform path from the lanes' lengths.
//             The tokens go to the workspace, their counts to LDS; the wave builds the three
//             Huffman codes (the two least keys merge, found by a wave-wide minimum), decides
//             between the dynamic and the stored block and writes the segment's bytes to its
//             own scratch range: 64 tokens a step, bit offsets from a wave scan, OR-ed in.
//   pack      one block per image: scan of the segment sizes, the Adler-32 combined in row
//             order (png.hip's rule), the capacity check, the copy behind the zlib header.
//
// Integer arithmetic only; the atomics are integer max/add in LDS and integer OR on words of
// the wave's own zeroed scratch: two runs are bit-equal.  Every write is bounded: a segment's
// block is stored whenever the dynamic one would not be smaller, so a segment's bytes never
// pass S + 10 of its S + 16 scratch bytes, and pack writes only streams that fit.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

namespace {

constexpr int kMaxImages = 4096;   // per call
constexpr int kMaxDim = 8192;
constexpr int kWave = 64;
constexpr int kHashBits = 12;
constexpr int kHash = 1 << kHashBits;
constexpr uint32_t kPrime = 4096;     // input bytes before a segment that are in the table at its start
constexpr uint32_t kWindow = 32768;
constexpr uint32_t kMaxMatch = 258;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr int kPackThreads = 256;
constexpr uint32_t kScratchSlack = 16;   // a segment's scratch: S + 16 bytes (at most S + 10 are used)

__constant__ unsigned char kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__host__ __device__ inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

struct Geo {
    uint32_t bpp, row_len, total, nseg;             // row_len and total count the filter bytes
    uint64_t rows, tokens, scratch, sizes, offs, bytes;   // offsets into the image's workspace range
};

__host__ __device__ inline Geo geometry(int h, int w, int kind, int s) {
    Geo g;
    g.bpp = kind == MD2_PNGENC_GRAY16 ? 2u : 3u;
    g.row_len = 1u + g.bpp * (uint32_t)w;
    g.total = (uint32_t)h * g.row_len;              // at most 8192 * 24577 < 2^32
    g.nseg = (g.total + (uint32_t)s - 1) / (uint32_t)s;
    g.rows = align_up(g.total, 16);
    g.tokens = g.rows + (uint64_t)h * 16;
    g.scratch = g.tokens + align_up((uint64_t)g.total * 4, 16);
    g.sizes = g.scratch + (uint64_t)g.nseg * ((uint32_t)s + kScratchSlack);
    g.offs = g.sizes + align_up((uint64_t)g.nseg * 4, 16);
    g.bytes = align_up(g.offs + align_up((uint64_t)g.nseg * 4, 16), 256);
    return g;
}

struct RowSums {
    uint32_t s1, pad;
    unsigned long long s2;
};

__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

template <typename T>
__device__ inline T wave_sum(T v) {
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ------------------------------------------------------------------ filter
__device__ inline uint32_t raw_byte(const uint8_t* in, int kind, uint32_t len, int r, uint32_t i) {
    if (kind != MD2_PNGENC_GRAY16) return in[(uint64_t)r * len + i];
    const uint32_t v = reinterpret_cast<const uint16_t*>(in)[(uint64_t)r * (len >> 1) + (i >> 1)];
    return (i & 1) ? (v & 255u) : (v >> 8);        // the samples big-endian
}

__device__ inline uint32_t paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

__device__ inline uint32_t predict(int ft, uint32_t a, uint32_t b, uint32_t c) {
    if (ft == 1) return a;
    if (ft == 2) return b;
    if (ft == 3) return (a + b) >> 1;
    if (ft == 4) return paeth((int)a, (int)b, (int)c);
    return 0;
}

__device__ inline uint32_t magnitude(uint32_t res) { return res < 128u ? res : 256u - res; }

__global__ __launch_bounds__(kWave) void pngenc_filter_kernel(const uint8_t* __restrict__ in,
                                                              const md2_pngenc_image* __restrict__ images,
                                                              uint8_t* __restrict__ workspace) {
    const md2_pngenc_image im = images[blockIdx.y];
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= im.height) return;
    const Geo g = geometry(im.height, im.width, im.kind, im.segment_bytes);
    const uint8_t* src = in + im.in_offset;
    uint8_t* ws = workspace + im.ws_offset;
    const uint32_t len = g.row_len - 1, bpp = g.bpp;
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (uint32_t i = lane; i < len; i += kWave) {
        const uint32_t x = raw_byte(src, im.kind, len, r, i);
        const uint32_t a = i >= bpp ? raw_byte(src, im.kind, len, r, i - bpp) : 0u;
        const uint32_t b = r ? raw_byte(src, im.kind, len, r - 1, i) : 0u;
        const uint32_t c = (r && i >= bpp) ? raw_byte(src, im.kind, len, r - 1, i - bpp) : 0u;
#pragma unroll
        for (int ft = 0; ft < 5; ++ft) cost[ft] += magnitude((x - predict(ft, a, b, c)) & 255u);
    }
    int best = 0;
    uint32_t least = 0;
#pragma unroll
    for (int ft = 0; ft < 5; ++ft) {
        const uint32_t t = wave_sum(cost[ft]);     // at most 3 * 8192 * 128
        if (ft == 0 || t < least) {
            least = t;
            best = ft;
        }
    }
    uint8_t* row = ws + (uint64_t)r * g.row_len;
    uint32_t s1 = 0;
    unsigned long long s2 = 0;
    if (lane == 0) {
        row[0] = (uint8_t)best;
        s1 = (uint32_t)best;
        s2 = (unsigned long long)g.row_len * (uint32_t)best;
    }
    for (uint32_t i = lane; i < len; i += kWave) {
        const uint32_t x = raw_byte(src, im.kind, len, r, i);
        const uint32_t a = i >= bpp ? raw_byte(src, im.kind, len, r, i - bpp) : 0u;
        const uint32_t b = r ? raw_byte(src, im.kind, len, r - 1, i) : 0u;
        const uint32_t c = (r && i >= bpp) ? raw_byte(src, im.kind, len, r - 1, i - bpp) : 0u;
        const uint32_t res = (x - predict(best, a, b, c)) & 255u;
        row[1 + i] = (uint8_t)res;
        s1 += res;
        s2 += (unsigned long long)(len - i) * res;   // byte j = 1 + i of the row weighs row_len - j
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        RowSums* rs = reinterpret_cast<RowSums*>(ws + g.rows) + r;
        rs->s1 = s1;
        rs->pad = 0;
        rs->s2 = s2;
    }
}

// ------------------------------------------------------------------ deflate
struct Lds {
    uint32_t table[kHash];          // hash -> 1 + the largest position inserted, 0: none
    uint32_t lit_freq[288], dist_freq[32], cl_freq[20];
    uint32_t work[288];             // the counts of one construction
    uint32_t key[576];              // count << 10 | node
    uint16_t parent[576];
    uint16_t lit_code[288], dist_code[32], cl_code[20];
    uint8_t lit_len[288], dist_len[32], cl_len[20];
    uint8_t op_sym[320], op_extra[320];
    uint32_t nops, hlit, hdist, hclen, header_bits;
};

__device__ inline uint32_t hash3(const uint8_t* d, uint32_t p) {
    const uint32_t v = d[p] | (uint32_t)d[p + 1] << 8 | (uint32_t)d[p + 2] << 16;
    return (v * 0x9E3779B1u) >> (32 - kHashBits);
}

__device__ inline uint32_t common(const uint8_t* d, uint32_t c, uint32_t p, uint32_t limit) {
    uint32_t n = 0;
    while (n < limit && d[c + n] == d[p + n]) ++n;
    return n;
}

__device__ inline void length_symbol(uint32_t len, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
    const uint32_t v = len - 3;
    if (v < 8) {
        sym = 257 + v, eb = 0, ev = 0;
    } else if (len == 258) {
        sym = 285, eb = 0, ev = 0;
    } else {
        eb = 29 - (uint32_t)__clz(v);              // bit_length - 3
        sym = 261 + 4 * eb + ((v >> eb) & 3u);
        ev = v & ((1u << eb) - 1u);
    }
}

__device__ inline void distance_symbol(uint32_t dist, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
    const uint32_t v = dist - 1;
    if (v < 4) {
        sym = v, eb = 0, ev = 0;
    } else {
        const uint32_t nb = 31 - (uint32_t)__clz(v);
        eb = nb - 1;
        sym = 2 * nb + ((v >> eb) & 1u);
        ev = v & ((1u << eb) - 1u);
    }
}

__device__ inline uint32_t lit_extra_bits(uint32_t sym) { return (sym < 265 || sym == 285) ? 0u : (sym - 261) >> 2; }
__device__ inline uint32_t dist_extra_bits(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1; }

__device__ inline uint32_t wave_min_key(const uint32_t* key, int nodes, int lane) {
    uint32_t m = kEmpty;
    for (int i = lane; i < nodes; i += kWave) m = min(m, key[i]);
    for (int d = kWave / 2; d > 0; d >>= 1) m = min(m, (uint32_t)__shfl_xor(m, d));
    return m;
}

// Code lengths of freq[0..nsym) (DESIGN.md §6n e): fewer than two used symbols count the
// lowest unused ones as 1; the two least (count, node) keys merge into node nsym + k; a code
// longer than `limit` halves every count upwards and starts again.
__device__ void build_lengths(Lds& s, const uint32_t* freq, int nsym, uint32_t limit, uint8_t* lens, int lane) {
    for (int i = lane; i < nsym; i += kWave) s.work[i] = freq[i];
    wave_sync();
    if (lane == 0) {
        int used = 0;
        for (int i = 0; i < nsym && used < 2; ++i) used += s.work[i] != 0;
        for (int i = 0; used < 2; ++i)
            if (s.work[i] == 0) {
                s.work[i] = 1;
                ++used;
            }
    }
    wave_sync();
    for (;;) {
        uint32_t leaves = 0;
        for (int i = lane; i < nsym; i += kWave) {
            const uint32_t c = s.work[i];
            s.key[i] = c ? (c << 10 | (uint32_t)i) : kEmpty;
            leaves += c != 0;
        }
        leaves = uniform(wave_sum(leaves));
        wave_sync();
        int nodes = nsym;
        for (uint32_t m = 1; m < leaves; ++m) {
            const uint32_t k1 = wave_min_key(s.key, nodes, lane);
            if (lane == 0) s.key[k1 & 1023u] = kEmpty;
            wave_sync();
            const uint32_t k2 = wave_min_key(s.key, nodes, lane);
            if (lane == 0) {
                s.key[k2 & 1023u] = kEmpty;
                s.key[nodes] = ((k1 >> 10) + (k2 >> 10)) << 10 | (uint32_t)nodes;
                s.parent[k1 & 1023u] = (uint16_t)nodes;
                s.parent[k2 & 1023u] = (uint16_t)nodes;
            }
            wave_sync();
            ++nodes;
        }
        const uint32_t root = (uint32_t)nodes - 1;
        uint32_t deepest = 0;
        for (int i = lane; i < nsym; i += kWave) {
            uint32_t depth = 0;
            if (s.work[i]) {
                uint32_t k = (uint32_t)i;
                while (k != root && depth < 576) {   // a leaf is at most 285 merges deep
                    k = s.parent[k];
                    ++depth;
                }
            }
            lens[i] = (uint8_t)depth;
            deepest = max(deepest, depth);
        }
        for (int d = kWave / 2; d > 0; d >>= 1) deepest = max(deepest, (uint32_t)__shfl_xor(deepest, d));
        wave_sync();
        if (uniform(deepest) <= limit) return;
        for (int i = lane; i < nsym; i += kWave)
            if (s.work[i]) s.work[i] = (s.work[i] + 1) >> 1;
        wave_sync();
    }
}

// RFC 1951's canonical codes, bit-reversed for the LSB-first writer.  One lane.
__device__ void canonical(const uint8_t* lens, int nsym, uint16_t* codes) {
    uint32_t count[16], next[16];
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int i = 0; i < nsym; ++i) ++count[lens[i]];
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (int i = 0; i < nsym; ++i) {
        const uint32_t n = lens[i];
        codes[i] = n ? (uint16_t)(__brev(next[n]++) >> (32 - n)) : (uint16_t)0;
    }
}

// `bits` (at most 48) of `pattern` OR-ed into the zeroed words at bit `pos`, inside `room` bits.
__device__ inline void put_bits(uint32_t* words, uint32_t pos, unsigned long long pattern, uint32_t bits,
                                uint32_t room) {
    if (bits == 0 || pos + bits > room) return;   // room: the scratch range in bits; never reached by the rules
    const uint32_t off = pos & 31u;
    uint32_t* w = words + (pos >> 5);
    const unsigned long long lo = pattern << off;
    atomicOr(w, (uint32_t)lo);
    if (off + bits > 32) atomicOr(w + 1, (uint32_t)(lo >> 32));
    if (off + bits > 64) atomicOr(w + 2, (uint32_t)(pattern >> (64 - off)));
}

__global__ __launch_bounds__(kWave) void pngenc_deflate_kernel(const md2_pngenc_image* __restrict__ images,
                                                               uint8_t* workspace) {
    __shared__ Lds s;
    const md2_pngenc_image im = images[blockIdx.y];
    const Geo g = geometry(im.height, im.width, im.kind, im.segment_bytes);
    const uint32_t seg = blockIdx.x;
    if (seg >= g.nseg) return;
    const int lane = threadIdx.x;
    const uint32_t S = (uint32_t)im.segment_bytes;
    uint8_t* ws = workspace + im.ws_offset;
    const uint8_t* d = ws;
    const uint32_t total = g.total;
    const uint32_t start = seg * S;
    const uint32_t end = min(total, start + S);
    const uint32_t n = end - start;
    const bool final = seg == g.nseg - 1;
    uint32_t* toks = reinterpret_cast<uint32_t*>(ws + g.tokens) + start;
    const uint32_t cap = S + kScratchSlack;
    uint8_t* scratch = ws + g.scratch + (uint64_t)seg * cap;
    uint32_t* words = reinterpret_cast<uint32_t*>(scratch);
    const uint32_t room = cap * 8;

    for (uint32_t i = lane; i < cap / 16; i += kWave) reinterpret_cast<uint4*>(scratch)[i] = make_uint4(0, 0, 0, 0);
    for (int i = lane; i < kHash; i += kWave) s.table[i] = 0;
    for (int i = lane; i < 288; i += kWave) s.lit_freq[i] = 0;
    if (lane < 32) s.dist_freq[lane] = 0;
    if (lane < 20) s.cl_freq[lane] = 0;
    wave_sync();

    // the table as the input before the segment leaves it
    for (uint32_t base = start > kPrime ? start - kPrime : 0; base < start; base += kWave) {
        const uint32_t p = base + lane;
        if (p < start && p + 3 <= total) atomicMax(&s.table[hash3(d, p)], p + 1);
    }
    wave_sync();

    uint32_t carry = 0;             // positions at the head of the step that a token already covers
    uint32_t ntok = 0;
    for (uint32_t base = start; base < end; base += kWave) {
        const uint32_t cnt = min((uint32_t)kWave, end - base);
        const uint32_t p = base + lane;
        const bool hashed = (uint32_t)lane < cnt && p + 3 <= total;
        const uint32_t h = hashed ? hash3(d, p) : 0u;
        uint32_t mlen = 0, mdist = 0;
        if (carry < cnt && (uint32_t)lane >= carry && (uint32_t)lane < cnt && p + 3 <= end) {
            const uint32_t limit = min(kMaxMatch, end - p);
            if (p >= 1) {
                mlen = common(d, p - 1, p, limit);
                mdist = 1;
            }
            const uint32_t c = s.table[h];
            if (c != 0 && p - (c - 1) <= kWindow) {
                const uint32_t m = common(d, c - 1, p, limit);
                if (m > mlen) {     // a tie stays with distance 1
                    mlen = m;
                    mdist = p - (c - 1);
                }
            }
        }
        wave_sync();
        if (hashed) atomicMax(&s.table[h], p + 1);
        wave_sync();
        if (carry >= cnt) {
            carry -= cnt;
            continue;
        }
        unsigned long long starts = 0;
        uint32_t pos = uniform(carry);
        while (pos < cnt) {
            const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)pos);
            starts |= 1ull << pos;
            pos = uniform(pos + (len >= 3 ? len : 1u));
        }
        carry = pos - cnt;
        if ((starts >> lane) & 1ull) {
            const uint32_t idx = ntok + (uint32_t)__popcll(starts & ((1ull << lane) - 1ull));
            uint32_t tok;
            if (mlen >= 3) {
                uint32_t sym, eb, ev;
                length_symbol(mlen, sym, eb, ev);
                atomicAdd(&s.lit_freq[sym], 1u);
                distance_symbol(mdist, sym, eb, ev);
                atomicAdd(&s.dist_freq[sym], 1u);
                tok = 0x80000000u | (mdist - 1) << 9 | (mlen - 3);
            } else {
                tok = d[p];
                atomicAdd(&s.lit_freq[tok], 1u);
            }
            toks[idx] = tok;        // idx < n: a token covers at least one byte
        }
        ntok += (uint32_t)__popcll(starts);
    }
    wave_sync();
    if (lane == 0) s.lit_freq[256] = 1;
    wave_sync();

    build_lengths(s, s.lit_freq, 286, 15, s.lit_len, lane);
    build_lengths(s, s.dist_freq, 30, 15, s.dist_len, lane);
    if (lane == 0) {
        uint32_t hlit = 286, hdist = 30;
        while (hlit > 257 && s.lit_len[hlit - 1] == 0) --hlit;
        while (hdist > 1 && s.dist_len[hdist - 1] == 0) --hdist;
        s.hlit = hlit;
        s.hdist = hdist;
        // the lengths run-length coded: at i a run of r equal values starts
        const uint32_t all = hlit + hdist;
        uint32_t nops = 0, i = 0, before = 0xFFu;
        while (i < all) {
            const uint32_t v = i < hlit ? s.lit_len[i] : s.dist_len[i - hlit];
            uint32_t r = 1;
            while (i + r < all && (i + r < hlit ? s.lit_len[i + r] : s.dist_len[i + r - hlit]) == v) ++r;
            uint32_t sym, extra, step;
            if (v == 0 && r >= 3) {
                step = min(r, 138u);
                sym = step >= 11 ? 18 : 17;
                extra = step >= 11 ? step - 11 : step - 3;
            } else if (v != 0 && before == v && r >= 3) {
                step = min(r, 6u);
                sym = 16;
                extra = step - 3;
            } else {
                step = 1;
                sym = v;
                extra = 0;
            }
            s.op_sym[nops] = (uint8_t)sym;
            s.op_extra[nops] = (uint8_t)extra;
            ++nops;
            ++s.cl_freq[sym];
            before = v;
            i += step;
        }
        s.nops = nops;
    }
    wave_sync();
    build_lengths(s, s.cl_freq, 19, 7, s.cl_len, lane);
    if (lane == 0) {
        uint32_t hclen = 19;
        while (hclen > 4 && s.cl_len[kOrder[hclen - 1]] == 0) --hclen;
        s.hclen = hclen;
        uint32_t bits = 17 + 3 * hclen;
        for (uint32_t i = 0; i < s.nops; ++i) {
            const uint32_t sym = s.op_sym[i];
            bits += s.cl_len[sym] + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
        }
        s.header_bits = bits;
    }
    wave_sync();
    uint32_t body = 0;
    for (int i = lane; i < 286; i += kWave) body += s.lit_freq[i] * (s.lit_len[i] + lit_extra_bits((uint32_t)i));
    if (lane < 30) body += s.dist_freq[lane] * (s.dist_len[lane] + dist_extra_bits((uint32_t)lane));
    const uint32_t bits = uniform(wave_sum(body)) + s.header_bits;
    uint32_t* sizes = reinterpret_cast<uint32_t*>(ws + g.sizes);
    __threadfence();                // the zeroed scratch is in place before any OR
    __builtin_amdgcn_wave_barrier();

    if ((bits + 7) / 8 >= n + 5) {  // stored: the dynamic block would not be smaller
        if (lane == 0) {
            scratch[0] = final ? 1 : 0;
            scratch[1] = (uint8_t)n;
            scratch[2] = (uint8_t)(n >> 8);
            scratch[3] = (uint8_t)~n;
            scratch[4] = (uint8_t)(~n >> 8);
            if (!final) {           // the empty stored block: 00, then 00 00 FF FF
                scratch[n + 8] = 0xFF;
                scratch[n + 9] = 0xFF;
            }
            sizes[seg] = n + 5 + (final ? 0u : 5u);
        }
        for (uint32_t i = lane; i < n; i += kWave) scratch[5 + i] = d[start + i];
        return;
    }

    uint32_t pos = 0;
    if (lane == 0) {
        canonical(s.lit_len, 286, s.lit_code);
        canonical(s.dist_len, 30, s.dist_code);
        canonical(s.cl_len, 19, s.cl_code);
        put_bits(words, pos, (final ? 1u : 0u) | 2u << 1, 3, room);
        put_bits(words, pos + 3, s.hlit - 257, 5, room);
        put_bits(words, pos + 8, s.hdist - 1, 5, room);
        put_bits(words, pos + 13, s.hclen - 4, 4, room);
        pos += 17;
        for (uint32_t i = 0; i < s.hclen; ++i, pos += 3) put_bits(words, pos, s.cl_len[kOrder[i]], 3, room);
        for (uint32_t i = 0; i < s.nops; ++i) {
            const uint32_t sym = s.op_sym[i];
            const uint32_t eb = sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u;
            put_bits(words, pos, s.cl_code[sym] | (unsigned long long)s.op_extra[i] << s.cl_len[sym],
                     s.cl_len[sym] + eb, room);
            pos += s.cl_len[sym] + eb;
        }
    }
    wave_sync();
    pos = s.header_bits;            // what lane 0 has written
    for (uint32_t t0 = 0; t0 < ntok; t0 += kWave) {
        unsigned long long pattern = 0;
        uint32_t nb = 0;
        if (t0 + lane < ntok) {
            const uint32_t tok = toks[t0 + lane];
            if (tok & 0x80000000u) {
                uint32_t sym, eb, ev;
                length_symbol((tok & 511u) + 3, sym, eb, ev);
                pattern = s.lit_code[sym];
                nb = s.lit_len[sym];
                pattern |= (unsigned long long)ev << nb;
                nb += eb;
                distance_symbol(((tok >> 9) & 0x7FFFu) + 1, sym, eb, ev);
                pattern |= (unsigned long long)s.dist_code[sym] << nb;
                nb += s.dist_len[sym];
                pattern |= (unsigned long long)ev << nb;
                nb += eb;           // at most 15 + 5 + 15 + 13
            } else {
                pattern = s.lit_code[tok];
                nb = s.lit_len[tok];
            }
        }
        uint32_t incl = nb;
        for (int dd = 1; dd < kWave; dd <<= 1) {
            const uint32_t y = __shfl_up(incl, dd);
            if (lane >= dd) incl += y;
        }
        put_bits(words, pos + incl - nb, pattern, nb, room);
        pos += (uint32_t)__shfl(incl, kWave - 1);
    }
    if (lane == 0) {
        put_bits(words, pos, s.lit_code[256], s.lit_len[256], room);
        pos += s.lit_len[256];      // == bits
        if (!final) {
            pos = (pos + 3 + 7) / 8 * 8;
            put_bits(words, pos, 0xFFFF0000u, 32, room);
            pos += 32;
        }
        sizes[seg] = (pos + 7) / 8;
    }
}

// ------------------------------------------------------------------ pack
__global__ __launch_bounds__(kPackThreads) void pngenc_pack_kernel(const md2_pngenc_image* __restrict__ images,
                                                                   uint8_t* workspace, uint8_t* out,
                                                                   uint32_t* __restrict__ stream_bytes,
                                                                   uint32_t* __restrict__ status) {
    __shared__ uint32_t wave_total[kPackThreads / kWave];
    __shared__ uint32_t fits;
    const md2_pngenc_image im = images[blockIdx.x];
    const Geo g = geometry(im.height, im.width, im.kind, im.segment_bytes);
    uint8_t* ws = workspace + im.ws_offset;
    const uint32_t* sizes = reinterpret_cast<const uint32_t*>(ws + g.sizes);
    uint32_t* offs = reinterpret_cast<uint32_t*>(ws + g.offs);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;   // the stream is at most total + 10 nseg + 6 < 2^32, kept wide for the check
    for (uint32_t base = 0; base < g.nseg; base += kPackThreads) {
        const uint32_t i = base + tid;
        const uint32_t v = i < g.nseg ? sizes[i] : 0u;
        uint32_t x = v;
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == kWave - 1) wave_total[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int k = 0; k < kPackThreads / kWave; ++k) {
            const uint32_t t = wave_total[k];
            if (k < wave) before += t;
            all += t;
        }
        if (i < g.nseg) offs[i] = (uint32_t)carry + before + (x - v);
        carry += all;
        __syncthreads();
    }
    const unsigned long long bytes = 2 + carry + 4;
    uint8_t* dst = out + im.out_offset;
    if (tid == 0) {
        stream_bytes[blockIdx.x] = (uint32_t)bytes;
        const bool ok = bytes <= im.out_capacity;
        status[blockIdx.x] = ok ? 0u : MD2_PNGENC_ST_SPACE;
        fits = ok;
        if (ok) {
            uint32_t a = 1, b = 0;  // png.hip's combine, rows in order
            const RowSums* rs = reinterpret_cast<const RowSums*>(ws + g.rows);
            for (int r = 0; r < im.height; ++r) {
                b = (uint32_t)((b + (unsigned long long)g.row_len * a + rs[r].s2 % 65521u) % 65521u);
                a = (a + rs[r].s1 % 65521u) % 65521u;
            }
            dst[0] = 0x78;          // deflate, 32 KiB window; FLG: no dictionary, check bits
            dst[1] = 0x01;
            uint8_t* t = dst + 2 + carry;
            t[0] = (uint8_t)(b >> 8);
            t[1] = (uint8_t)b;
            t[2] = (uint8_t)(a >> 8);
            t[3] = (uint8_t)a;
        }
    }
    __syncthreads();                // also: offs are visible to the block
    if (!fits) return;              // does not fit: nothing of the range is written
    const uint32_t cap = (uint32_t)im.segment_bytes + kScratchSlack;
    for (uint32_t sg = wave; sg < g.nseg; sg += kPackThreads / kWave) {
        const uint8_t* src = ws + g.scratch + (uint64_t)sg * cap;
        uint8_t* to = dst + 2 + offs[sg];
        const uint32_t nb = sizes[sg];
        for (uint32_t k = lane; k < nb; k += kWave) to[k] = src[k];
    }
}

// ------------------------------------------------------------------ host
const char* check_images(const md2_pngenc_image* images, int n) {
    if (!images) return "png encode: images is NULL";
    if (n < 1 || n > kMaxImages) return "png encode: n must be 1..4096";
    for (int i = 0; i < n; ++i) {
        const md2_pngenc_image& im = images[i];
        if (im.height < 1 || im.height > kMaxDim || im.width < 1 || im.width > kMaxDim)
            return "png encode: height and width must be 1..8192";
        if (im.kind != MD2_PNGENC_RGB8 && im.kind != MD2_PNGENC_GRAY16) return "png encode: unknown kind";
        const int s = im.segment_bytes;
        if (s < 1024 || s > 32768 || (s & (s - 1)))
            return "png encode: segment_bytes must be a power of two in 1024..32768";
    }
    return nullptr;
}

size_t stream_bound(const md2_pngenc_image& im) {
    const Geo g = geometry(im.height, im.width, im.kind, im.segment_bytes);
    return (size_t)g.total + 10 * (size_t)g.nseg + 6;
}

size_t workspace_need(const md2_pngenc_image* images, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i)
        total += geometry(images[i].height, images[i].width, images[i].kind, images[i].segment_bytes).bytes;
    return total;
}

const char* check_ranges(const md2_pngenc_image* images, int n, uint64_t in_bytes, uint64_t out_bytes) {
    uint64_t ws = 0;
    for (int i = 0; i < n; ++i) {
        const md2_pngenc_image& im = images[i];
        const Geo g = geometry(im.height, im.width, im.kind, im.segment_bytes);
        const uint64_t ib = (uint64_t)im.height * im.width * g.bpp;
        if (im.in_offset > in_bytes || ib > in_bytes - im.in_offset) return "png encode: a frame reaches past in_bytes";
        if (im.kind == MD2_PNGENC_GRAY16 && im.in_offset % 2)
            return "png encode: a 16-bit frame's in_offset must be a multiple of 2";
        if (im.out_offset > out_bytes || im.out_capacity > out_bytes - im.out_offset)
            return "png encode: an output range reaches past out_bytes";
        if (im.ws_offset != ws) return "png encode: ws_offset must be the sum of the workspace ranges before the image";
        if (im.reserved != 0) return "png encode: reserved must be 0";
        ws += g.bytes;
    }
    return nullptr;
}

}  // namespace

extern "C" {

size_t md2_png_encode_bound(int height, int width, int kind, int segment_bytes) {
    md2_pngenc_image im = {};
    im.height = height;
    im.width = width;
    im.kind = kind;
    im.segment_bytes = segment_bytes;
    if (const char* msg = check_images(&im, 1)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return stream_bound(im);
}

size_t md2_png_encode_workspace_bytes(const md2_pngenc_image* images, int n) {
    if (const char* msg = check_images(images, n)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return workspace_need(images, n);
}

int md2_png_encode_check(const md2_pngenc_image* images, int n, uint64_t in_bytes, uint64_t out_bytes) {
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, in_bytes, out_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    return MD2_OK;
}

int md2_png_encode(const uint8_t* in, uint64_t in_bytes, const md2_pngenc_image* images,
                   const md2_pngenc_image* dev_images, int n, void* workspace, size_t workspace_bytes, uint8_t* out,
                   uint64_t out_bytes, uint32_t* stream_bytes, uint32_t* status, void* stream) {
    if (!in || !images || !dev_images || !workspace || !out || !stream_bytes || !status)
        return md2_report_error(MD2_ERR_ARG,
                                "png encode: in/images/dev_images/workspace/out/stream_bytes/status is NULL");
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, in_bytes, out_bytes)) return md2_report_error(MD2_ERR_ARG, msg);
    if (reinterpret_cast<uintptr_t>(in) % 2 || reinterpret_cast<uintptr_t>(workspace) % 256 ||
        reinterpret_cast<uintptr_t>(dev_images) % 8)
        return md2_report_error(MD2_ERR_ARG,
                                "png encode: in must be 2-byte, workspace 256-byte, dev_images 8-byte aligned");
    if (workspace_need(images, n) > workspace_bytes)
        return md2_report_error(MD2_ERR_ARG, "png encode: the batch needs more workspace than workspace_bytes");
    uint32_t max_h = 1, max_seg = 1;
    for (int i = 0; i < n; ++i) {
        const Geo g = geometry(images[i].height, images[i].width, images[i].kind, images[i].segment_bytes);
        if ((uint32_t)images[i].height > max_h) max_h = (uint32_t)images[i].height;
        if (g.nseg > max_seg) max_seg = g.nseg;
    }
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    hipLaunchKernelGGL(pngenc_filter_kernel, dim3(max_h, n), dim3(kWave), 0, st, in, dev_images, ws);
    hipLaunchKernelGGL(pngenc_deflate_kernel, dim3(max_seg, n), dim3(kWave), 0, st, dev_images, ws);
    hipLaunchKernelGGL(pngenc_pack_kernel, dim3(n), dim3(kPackThreads), 0, st, dev_images, ws, out, stream_bytes,
                       status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
