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
    __device__ uint4 load(uint32_t chunk) const {
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
    __device__ void store(uint32_t half, uint4 v) { reinterpret_cast<uint4*>(in)[(half & 1) * kWave + lane] = v; }

    __device__ void refill() {
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
    __device__ void seek(uint32_t byte) {
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
__device__ int decode(const Huff& h, Reader& br) {
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

__global__ __launch_bounds__(kWave) void png_inflate_kernel(const uint8_t* __restrict__ streams,
                                                            const md2_png_image* __restrict__ images,
                                                            uint8_t* __restrict__ workspace,
                                                            uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
    __shared__ __attribute__((aligned(16))) uint32_t in[kInWords];
    __shared__ Huff lit, dst;
    __shared__ uint8_t lens[320];
    __shared__ uint8_t cl_lens[19];
    __shared__ uint16_t codes[320];
    __shared__ uint16_t work[32];

    const int img = blockIdx.x, lane = threadIdx.x;
    const md2_png_image im = images[img];
    const uint32_t total = (uint32_t)raw_bytes(im.height, im.width);
    uint8_t* ws = workspace + workspace_offset(images, img, lane);

    Reader br;
    br.src = streams + im.stream_offset;
    br.nbytes = im.stream_bytes;
    br.in = in;
    br.lane = lane;
    br.seek(0);

    uint32_t pos = 0, flushed = 0, st = 0;

    // the ring's bytes [flushed, upto) to the workspace; upto is a multiple of 16, at most align16(total)
    auto flush = [&](uint32_t upto) {
        wave_sync();
        for (uint32_t o = flushed + 16u * lane; o < upto; o += 16u * kWave)
            *reinterpret_cast<uint4*>(ws + o) = *reinterpret_cast<const uint4*>(ring + (o & kRingMask));
        flushed = upto;
    };

    while (true) {
        br.refill();
        const uint32_t last = br.bits(1), type = br.bits(2);
        if (type == 3) {
            st = MD2_PNG_ST_BLOCK;
            break;
        }
        if (type == 0) {
            br.drop(br.bc & 7);
            br.refill();
            const uint32_t len = br.bits(16);
            br.refill();
            const uint32_t nlen = br.bits(16);
            if (br.overrun()) break;
            if ((len ^ 0xFFFFu) != nlen) {
                st = MD2_PNG_ST_BLOCK;
                break;
            }
            if (len) {
                uint32_t byte = (uint32_t)(br.consumed() >> 3);
                const uint32_t have = br.nbytes - byte;            // no overrun: byte <= nbytes
                uint32_t n = len < have ? len : have;
                if (n > total - pos) n = total - pos;
                const uint32_t end = byte + len;
                while (n) {
                    const uint32_t piece = n < kFlush ? n : kFlush;
                    wave_sync();
                    for (uint32_t i = lane; i < piece; i += kWave) ring[(pos + i) & kRingMask] = br.src[byte + i];
                    pos += piece;
                    byte += piece;
                    n -= piece;
                    if (pos - flushed >= kFlush) flush(pos & ~15u);
                }
                if (pos >= total) break;
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
            while (true) {
                br.refill();
                int sym = decode(lit, br);
                if (sym < 0) {
                    st = br.no_code();
                    break;
                }
                if (sym < 256) {
                    if (lane == 0) ring[pos & kRingMask] = (uint8_t)sym;
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
                    if (len > total - pos) len = total - pos;
                    const uint32_t from = pos - dist;
                    wave_sync();
                    if (dist >= len) {
                        for (uint32_t i = lane; i < len; i += kWave)
                            ring[(pos + i) & kRingMask] = ring[(from + i) & kRingMask];
                    } else {   // the copy repeats a period: byte i is source byte i mod dist
                        for (uint32_t i = lane; i < len; i += kWave)
                            ring[(pos + i) & kRingMask] = ring[(from + i % dist) & kRingMask];
                    }
                    wave_sync();
                    pos += len;
                }
                if (pos >= total || br.overrun()) break;
                if (pos - flushed >= kFlush) flush(pos & ~15u);
            }
            if (st) break;
        }
        if (pos >= total || br.overrun()) break;
        if (last) {
            st = MD2_PNG_ST_END;   // the last block ends before the image is complete
            break;
        }
        if (pos - flushed >= kFlush) flush(pos & ~15u);
    }
    if (br.overrun()) st = MD2_PNG_ST_END;   // whatever the zeros past the end decoded to
    flush((uint32_t)align16(pos));
    if (lane == 0) status[img] = st;
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

const char* check_ranges(const md2_png_image* images, int n, uint64_t streams_bytes, uint64_t out_bytes) {
    for (int i = 0; i < n; ++i) {
        const md2_png_image& im = images[i];
        if (im.stream_offset % 16 || im.out_offset % 16) return "png: stream_offset and out_offset must be multiples of 16";
        if (im.stream_offset > streams_bytes || im.stream_bytes > streams_bytes - im.stream_offset)
            return "png: a stream reaches past streams_bytes";
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

}  // namespace

extern "C" {

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
