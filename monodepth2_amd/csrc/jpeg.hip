// jpeg.hip — baseline JPEG decoding on gfx950 for training from disk: the compressed
// frames of a batch -> the tight (h, w, 3) RGB bytes md2_aug_run_mixed reads, every byte
// what Pillow (libjpeg's accurate-integer path) gives for the file.
//
// The host parses the headers and hands over the entropy-coded segment with the byte
// stuffing removed (monodepth2_amd/jpeg_ops.py); md2_jpeg_run (include/md2hot.h) is a fixed
// chain of launches for the whole batch, the image on grid.y / grid.x:
//
//   memset      the coefficient planes (an end-of-block leaves zeros)
//   entropy     one workgroup per image: Huffman tables into LDS, the subsequence entry
//               states by fixed-point iteration, blocks per subsequence, a workgroup scan,
//               then the coefficients de-zigzagged as int16 into per-component planes
//   dc          per (image, component): inclusive scan of the DC differences in MCU order
//   idct        one thread per 8x8 block: dequantise, jidctint's islow transform, +128,
//               clamp -> uint8 sample planes
//   colour      one thread per pixel: chroma upsampling (libjpeg's fancy filters and its
//               narrow-plane replication) and YCbCr -> RGB, three bytes at the image's offset
//
// Entropy decoding without restart markers.  The unstuffed stream is cut into subsequences
// of kSubBits bits.  Slot i holds the decoder state at the first symbol that starts at or
// after bit kSubBits * i: (bit position, block within the MCU, zigzag index), one 64-bit
// word.  Slot 0 is the truth (0, 0, 0); slot i starts as the guess (kSubBits * i, 0, 0).  A
// round decodes every subsequence whose entry slot was written in the round before from that
// slot and writes its exit state to the next slot when it differs; rounds are separated by
// workgroup barriers and end with a round that writes nothing.  Slot i + 1 is then the decode
// of subsequence i from slot i for every i, and slot 0 is true, so the slots are those of
// the sequential decode: the fixed point is unique.  After round r slots 0..r are final, so
// there are at most N + 1 rounds.  A subsequence may read its entry slot while the thread
// of the one before writes it in the same round (64-bit relaxed atomics: never torn): every
// write is followed by a decode of that subsequence in a later round, so the order in which
// the hardware runs the threads changes the number of rounds, never the result.
//
// Decoding from a guessed state reads garbage, so that is the normal case, not an error
// path: bit fetches past the stream return zeros, a Huffman miss advances 16 bits, a zigzag
// index past 63 ends the block, coefficient writes happen only in the final pass and only
// for blocks below the image's block count, and every loop advances the bit position.
//
// The slots the iteration ends with are a property of the file.  md2_jpeg_index runs the
// iteration alone and writes them out with the blocks completed before each (the index);
// md2_jpeg_run_indexed replaces `entropy` by jpeg_entropy_indexed_kernel, which starts every
// subsequence of every image from its stored slot: workgroups over (image, group of
// subsequences), no rounds, and every exit state checked against the next stored one.
//
// Integer arithmetic only; no atomics on coefficients, samples or pixels (the status word
// takes an atomic OR).  Products that a corrupt stream can push past 32 bits wrap (-fwrapv).

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <new>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

namespace {

constexpr int kThreads = 1024;        // entropy and dc workgroups
constexpr int kIxThreads = 256;       // indexed entropy workgroups
constexpr int kSubBits = 1024;        // bits per subsequence (128 bytes)
constexpr int kFastBits = 9;          // Huffman codes up to this length: one LDS lookup
constexpr int kRing = 4;              // pinned descriptor slots per plan
constexpr int kMaxImages = 4096;      // per call
constexpr int kMaxDim = 8192;
constexpr uint32_t kMaxStream = 1u << 28;   // bytes: bit positions stay below 2^31
constexpr int kHuffBytes = 272;       // counts[16], values[256]

constexpr uint32_t kStShort = MD2_JPEG_ST_BLOCKS;
constexpr uint32_t kStCode = MD2_JPEG_ST_CODE;
constexpr uint32_t kStEnd = MD2_JPEG_ST_END;
constexpr uint32_t kStIndex = MD2_JPEG_ST_INDEX;

__device__ const unsigned char kZigzag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Img {                  // one image of the batch, on the device
    const uint32_t* words;    // the unstuffed stream, 4-byte aligned
    uint32_t nbytes;
    int h, w, hs, vs;         // luma sampling factors (chroma is 1 x 1)
    int mcux, mcuy;
    int bpm;                  // blocks per MCU
    uint32_t total_blocks;
    int qt[3], dct[3], act[3];
    int wb[3], hb[3];         // component plane in blocks
    int16_t* coef[3];
    uint8_t* plane[3];        // samples, (hb * 8) rows of (wb * 8)
    unsigned long long* slots;   // nsub + 1
    uint32_t* dirty;             // nsub + 1: the round in which the slot was last written
    uint32_t* counts;            // nsub: blocks completed in the subsequence
    uint32_t nsub;
    uint8_t* out;
    uint32_t* status;
    unsigned long long* ix_state;   // md2_jpeg_index / md2_jpeg_run_indexed: nsub entry states
    uint32_t* ix_first;             // and nsub counts of the blocks completed before them
};

struct Huff {                 // one table in LDS
    uint16_t fast[1 << kFastBits];   // len << 8 | symbol, 0 = longer than kFastBits or no code
    int maxcode[17];                 // largest code of each length, -1 = none
    int base[17];                    // valptr - mincode
    uint8_t vals[256];
};

struct Bits {                 // big-endian bit reader over aligned words, zero past the end
    const uint32_t* w;
    uint32_t nwords, tailmask, wp;
    unsigned long long win;

    __device__ __forceinline__ uint32_t word(uint32_t i) const {
        if (i >= nwords) return 0u;
        uint32_t v = __builtin_bswap32(w[i]);
        if (i == nwords - 1) v &= tailmask;
        return v;
    }
    __device__ __forceinline__ void init(const Img& im) {
        w = im.words;
        nwords = (im.nbytes + 3) >> 2;
        const uint32_t r = im.nbytes & 3u;
        tailmask = r ? ~(0xFFFFFFFFu >> (8 * r)) : 0xFFFFFFFFu;
        wp = 0xFFFFFFFFu;
        win = 0;
    }
    // the 32 bits starting at bit p
    __device__ __forceinline__ uint32_t peek(uint32_t p) {
        const uint32_t i = p >> 5;
        if (i != wp) {
            wp = i;
            win = ((unsigned long long)word(i) << 32) | word(i + 1);
        }
        return (uint32_t)((win << (p & 31u)) >> 32);
    }
};

__device__ __forceinline__ unsigned long long pack_state(uint32_t p, uint32_t b, uint32_t k) {
    return ((unsigned long long)p << 16) | (b << 8) | k;
}

__device__ __forceinline__ unsigned long long slot_load(const unsigned long long* s) {
    return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void slot_store(unsigned long long* s, unsigned long long v) {
    __hip_atomic_store(s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// component of block b of an MCU, and its index within the component's blocks of the MCU
__device__ __forceinline__ void block_comp(const Img& im, uint32_t b, int& c, int& jc) {
    const int ny = im.hs * im.vs;
    if ((int)b < ny) { c = 0; jc = (int)b; }
    else { c = (int)b - ny + 1; jc = 0; }
    if (c > 2) c = 2;   // unreachable for b < bpm; keeps a table index inside whatever b is
}

// the coefficients of block g (block b of its MCU), nullptr at or past the image's blocks
__device__ __forceinline__ int16_t* block_ptr(const Img& im, uint32_t g, uint32_t b) {
    if (g >= im.total_blocks) return nullptr;
    int c, jc;
    block_comp(im, b, c, jc);
    const uint32_t m = g / (uint32_t)im.bpm;
    const int mx = (int)(m % (uint32_t)im.mcux), my = (int)(m / (uint32_t)im.mcux);
    const int hs = c ? 1 : im.hs, vs = c ? 1 : im.vs;
    const int bx = mx * hs + jc % hs, by = my * vs + jc / hs;
    if (bx >= im.wb[c] || by >= im.hb[c]) return nullptr;   // unreachable for g < total_blocks
    return im.coef[c] + ((size_t)by * im.wb[c] + bx) * 64;
}

// Decodes from `state` until the bit position reaches `end` (or the stream's end); returns
// the blocks completed.  WRITE: block g0 + n goes to its plane, nothing is decoded at or past
// the image's block count, and `flags` collects what went wrong.
template <bool WRITE>
__device__ uint32_t decode_range(const Img& im, const Huff* tabs, Bits& bits, unsigned long long& state, uint32_t end,
                                 uint32_t g0, uint32_t& flags) {
    const uint32_t total_bits = im.nbytes * 8u;
    if (end > total_bits) end = total_bits;
    uint32_t p = (uint32_t)(state >> 16), b = (uint32_t)(state >> 8) & 255u, k = (uint32_t)state & 255u;
    if ((int)b >= im.bpm) b = 0;   // slots are written by this kernel only; keeps garbage harmless
    if (k > 63) k = 0;
    uint32_t done = 0;
    int c, jc;
    block_comp(im, b, c, jc);
    int16_t* dst = WRITE ? block_ptr(im, g0, b) : nullptr;
    while (p < end) {
        if (WRITE && g0 + done >= im.total_blocks) break;
        const Huff& H = tabs[2 * c + (k ? 1 : 0)];
        const uint32_t look = bits.peek(p);
        const uint32_t code16 = look >> 16;
        uint32_t len, sym;
        const uint32_t e = H.fast[code16 >> (16 - kFastBits)];
        if (e) {
            len = e >> 8;
            sym = e & 255u;
        } else {
            len = 16;
            sym = 0;
            bool hit = false;
            for (int l = kFastBits + 1; l <= 16; ++l) {
                const int code = (int)(code16 >> (16 - l));
                if (code <= H.maxcode[l]) {
                    len = (uint32_t)l;
                    sym = H.vals[(H.base[l] + code) & 255];
                    hit = true;
                    break;
                }
            }
            if (!hit && WRITE) flags |= kStCode;   // a miss: 16 bits, symbol 0
        }
        const uint32_t s = k ? (sym & 15u) : (sym > 15u ? 15u : sym);
        if (p + len + s > total_bits) {   // the symbol leaves the stream: nothing more to decode
            if (WRITE) flags |= kStEnd;
            p = total_bits;
            break;
        }
        int v = 0;
        if (s) {
            const uint32_t raw = (look << len) >> (32 - s);
            v = raw < (1u << (s - 1)) ? (int)raw - (int)(1u << s) + 1 : (int)raw;
        }
        p += len + s;
        bool block_done = false;
        if (k == 0) {
            if (WRITE && dst) dst[0] = (int16_t)v;   // the DC difference; summed by the dc kernel
            k = 1;
        } else {
            const uint32_t r = sym >> 4;
            if (s == 0) {
                if (r == 15) k += 16;       // ZRL
                else block_done = true;     // EOB (r below 15 with no bits is an end of block here)
            } else {
                k += r;
                if (k <= 63) {
                    if (WRITE && dst) dst[kZigzag[k]] = (int16_t)v;
                    ++k;
                }
            }
            if (k > 63) block_done = true;
        }
        if (block_done) {
            ++done;
            k = 0;
            b = (int)(b + 1) >= im.bpm ? 0 : b + 1;
            block_comp(im, b, c, jc);
            if (WRITE) dst = block_ptr(im, g0 + done, b);
        }
    }
    state = pack_state(p, b, k);
    return done;
}

// LDS tables of the image's six (component, DC / AC) pairs from the bank's counts and values,
// by a workgroup of STRIDE threads (at least 6)
template <int STRIDE>
__device__ void build_tables(const Img& im, const uint8_t* huff, int num_huff, Huff* tabs) {
    const int t = threadIdx.x;
    for (int i = t; i < 6 * (1 << kFastBits); i += STRIDE) tabs[i >> kFastBits].fast[i & ((1 << kFastBits) - 1)] = 0;
    if (t < 6) {
        int id = (t & 1) ? im.act[t >> 1] : im.dct[t >> 1];
        id = id < 0 ? 0 : (id >= num_huff ? num_huff - 1 : id);
        const uint8_t* src = huff + (size_t)id * kHuffBytes;
        Huff& H = tabs[t];
        int code = 0, ptr = 0;
        for (int l = 1; l <= 16; ++l) {
            const int n = src[l - 1];
            H.base[l] = ptr - code;
            H.maxcode[l] = n ? code + n - 1 : -1;
            if (H.maxcode[l] >= (1 << l)) H.maxcode[l] = (1 << l) - 1;   // an oversubscribed length
            code = (code + n) << 1;
            ptr += n;
        }
        H.maxcode[0] = -1;
        H.base[0] = 0;
    }
    for (int i = t; i < 6 * 256; i += STRIDE) {
        const int id0 = ((i >> 8) & 1) ? im.act[i >> 9] : im.dct[i >> 9];
        const int id = id0 < 0 ? 0 : (id0 >= num_huff ? num_huff - 1 : id0);
        tabs[i >> 8].vals[i & 255] = huff[(size_t)id * kHuffBytes + 16 + (i & 255)];
    }
    __syncthreads();
    // symbol j of table q: its length and code, then every lookup entry it prefixes
    for (int i = t; i < 6 * 256; i += STRIDE) {
        const int q = i >> 8, j = i & 255;
        const int id0 = (q & 1) ? im.act[q >> 1] : im.dct[q >> 1];
        const int id = id0 < 0 ? 0 : (id0 >= num_huff ? num_huff - 1 : id0);
        const uint8_t* cnt = huff + (size_t)id * kHuffBytes;
        Huff& H = tabs[q];
        int ptr = 0;
        for (int l = 1; l <= kFastBits; ++l) {
            const int n = cnt[l - 1];
            if (j < ptr + n) {
                const int code = j - H.base[l];
                if (code < (1 << l)) {
                    const int first = code << (kFastBits - l), span = 1 << (kFastBits - l);
                    for (int x = 0; x < span; ++x) H.fast[first + x] = (uint16_t)((l << 8) | H.vals[j]);
                }
                break;
            }
            ptr += n;
        }
    }
    __syncthreads();
}

// inclusive scan of one value per thread over the workgroup, fixed shape; returns the
// exclusive prefix and leaves the total in *total
__device__ uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const uint32_t o = t >= d ? lds[t - d] : 0u;
        __syncthreads();
        lds[t] += o;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[kThreads - 1];
    __syncthreads();
    return incl - v;
}

// grid: images.  INDEX: the synchronisation alone; the final slots and the blocks before each
// go to the image's index and nothing is decoded for real (md2_jpeg_index).
template <bool INDEX>
__global__ __launch_bounds__(kThreads) void jpeg_entropy_kernel(const Img* imgs, const uint8_t* huff, int num_huff) {
    __shared__ Huff tabs[6];
    __shared__ uint32_t scan[kThreads];
    const Img& im = imgs[blockIdx.x];
    const int t = threadIdx.x;
    build_tables<kThreads>(im, huff, num_huff, tabs);
    for (uint32_t i = t; i <= im.nsub; i += kThreads) {
        slot_store(&im.slots[i], pack_state(i * (uint32_t)kSubBits, 0, 0));
        im.dirty[i] = 0;
    }
    if (t == 0) *im.status = 0;
    __syncthreads();
    Bits bits;
    bits.init(im);
    uint32_t flags = 0;
    // rounds: a subsequence is decoded again when its entry slot was written in the round before
    for (uint32_t round = 1;; ++round) {
        int wrote = 0;
        for (uint32_t i = t; i < im.nsub; i += kThreads) {
            if (__hip_atomic_load(&im.dirty[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != round - 1) continue;
            unsigned long long st = slot_load(&im.slots[i]);
            im.counts[i] = decode_range<false>(im, tabs, bits, st, (i + 1) * (uint32_t)kSubBits, 0, flags);
            if (st != slot_load(&im.slots[i + 1])) {   // slot i + 1 has this one writer
                slot_store(&im.slots[i + 1], st);
                __hip_atomic_store(&im.dirty[i + 1], round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                wrote = 1;
            }
        }
        __threadfence_block();
        if (!__syncthreads_or(wrote)) break;
    }
    // blocks before each thread's run of consecutive subsequences
    const uint32_t chunk = (im.nsub + kThreads - 1) / kThreads;
    const uint32_t first = (uint32_t)t * chunk;
    const uint32_t last = first + chunk < im.nsub ? first + chunk : im.nsub;
    uint32_t mine = 0;
    for (uint32_t i = first; i < last; ++i) mine += im.counts[i];
    uint32_t total;
    uint32_t g = block_scan(mine, scan, &total);
    if (INDEX) {
        for (uint32_t i = first; i < last; ++i) {
            im.ix_state[i] = slot_load(&im.slots[i]);
            im.ix_first[i] = g;
            g += im.counts[i];
        }
        // the index is padded to 16 bytes: 12 * nsub bytes, then (nsub & 3) words of zeros
        if ((uint32_t)t < (im.nsub & 3u)) im.ix_first[im.nsub + t] = 0;
        if (t == 0 && total != im.total_blocks) atomicOr(im.status, kStShort);
        return;
    }
    for (uint32_t i = first; i < last; ++i) {
        unsigned long long st = slot_load(&im.slots[i]);
        const uint32_t n = im.counts[i];
        if (g < im.total_blocks) decode_range<true>(im, tabs, bits, st, (i + 1) * (uint32_t)kSubBits, g, flags);
        g += n;
    }
    if (t == 0 && total != im.total_blocks) flags |= kStShort;
    if (flags) atomicOr(im.status, flags);
}

// grid (ceil(max nsub / kIxThreads), images): the entropy decode from a stored index
// (md2_jpeg_run_indexed).  A workgroup belongs to one image and builds its tables; thread t
// then decodes subsequence i = blockIdx.x * kIxThreads + t from ix_state[i] with ix_first[i]
// blocks before it, independently of every other: no barrier after the table build, no slot
// memory, no atomic but the status word's (cleared by a memset before the launch, since
// several workgroups share it).  One subsequence per thread: a KITTI batch has about one
// wave per SIMD of them, and two or four per thread measured 1.24 and 1.89 times the chain's
// time.
//
// The index is not trusted.  An entry state must be 0 for subsequence 0 and otherwise hold a
// bit position in [kSubBits * i, stream bits]: anything else is reported and not decoded, so
// a thread never decodes more than its kSubBits bits.  After the decode, with g1 = ix_first[i]
// + blocks completed: while g1 is below the image's block count, the exit state must equal
// ix_state[i + 1] and g1 must equal ix_first[i + 1]; once the image's blocks are complete
// (the decode stops there, the synchronisation that made the index did not, so their states
// may differ) ix_first[i + 1] must not be below the block count either; the last subsequence
// must end at exactly the block count.  A mismatch sets MD2_JPEG_ST_INDEX (with _BLOCKS for
// the last subsequence).  Writes are clamped to the image's own planes by block_ptr and
// decode_range whatever the index says.
__global__ __launch_bounds__(kIxThreads) void jpeg_entropy_indexed_kernel(const Img* imgs, const uint8_t* huff,
                                                                          int num_huff) {
    __shared__ Huff tabs[6];
    const Img& im = imgs[blockIdx.y];
    if (blockIdx.x * (uint32_t)kIxThreads >= im.nsub) return;   // the whole workgroup: the grid is the largest image's
    build_tables<kIxThreads>(im, huff, num_huff, tabs);
    const uint32_t i = blockIdx.x * (uint32_t)kIxThreads + threadIdx.x;
    if (i >= im.nsub) return;
    Bits bits;
    bits.init(im);
    const uint32_t total_bits = im.nbytes * 8u;
    unsigned long long st = im.ix_state[i];
    const uint32_t g0 = im.ix_first[i];
    const uint32_t p = (uint32_t)(st >> 16);
    if ((st >> 48) || p < i * (uint32_t)kSubBits || p > total_bits || (i == 0 && (st || g0))) {
        atomicOr(im.status, kStIndex);
        return;
    }
    uint32_t flags = 0, done = 0;
    if (g0 < im.total_blocks) done = decode_range<true>(im, tabs, bits, st, (i + 1) * (uint32_t)kSubBits, g0, flags);
    const uint32_t g1 = g0 + done;
    if (i + 1 == im.nsub) {
        if (g1 != im.total_blocks) flags |= kStIndex | kStShort;
    } else {
        const uint32_t next = im.ix_first[i + 1];
        if (g1 < im.total_blocks) {
            if (st != im.ix_state[i + 1] || g1 != next) flags |= kStIndex;
        } else if (next < im.total_blocks) {
            flags |= kStIndex;
        }
    }
    if (flags) atomicOr(im.status, flags);
}

// grid (3, images): the DC differences of a component summed in decode order
__global__ __launch_bounds__(kThreads) void jpeg_dc_kernel(const Img* imgs) {
    __shared__ uint32_t scan[kThreads];
    const Img& im = imgs[blockIdx.y];
    const int c = blockIdx.x, t = threadIdx.x;
    const int hs = c ? 1 : im.hs, vs = c ? 1 : im.vs, nb = hs * vs;
    const uint32_t n = (uint32_t)im.mcux * im.mcuy * nb;
    const uint32_t chunk = (n + kThreads - 1) / kThreads;
    const uint32_t first = (uint32_t)t * chunk, last = first + chunk < n ? first + chunk : n;
    auto at = [&](uint32_t s) -> int16_t* {
        const uint32_t m = s / (uint32_t)nb;
        const int jc = (int)(s % (uint32_t)nb);
        const int bx = (int)(m % (uint32_t)im.mcux) * hs + jc % hs, by = (int)(m / (uint32_t)im.mcux) * vs + jc / hs;
        return im.coef[c] + ((size_t)by * im.wb[c] + bx) * 64;
    };
    uint32_t mine = 0;
    for (uint32_t s = first; s < last; ++s) mine += (uint32_t)(int)*at(s);
    uint32_t total;
    uint32_t run = block_scan(mine, scan, &total);
    for (uint32_t s = first; s < last; ++s) {
        int16_t* p = at(s);
        run += (uint32_t)(int)*p;
        *p = (int16_t)run;
    }
}

constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270;
constexpr int FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137;
constexpr int FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

// the eight-point accurate-integer inverse DCT of one column / row: in[0..7] -> out[0..7],
// descaled by `shift` with rounding (CONST_BITS = 13)
__device__ __forceinline__ void idct8(const int* in, int* out, int shift) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * FIX_0_541196100;
    const int tmp2 = z1 + z3 * (-FIX_1_847759065);
    const int tmp3 = z1 + z2 * FIX_0_765366865;
    z2 = in[0];
    z3 = in[4];
    const int tmp0 = (z2 + z3) * 8192;   // << CONST_BITS
    const int tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    z1 = t0 + t3;
    z2 = t1 + t2;
    z3 = t0 + t2;
    int z4 = t1 + t3;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    t0 *= FIX_0_298631336;
    t1 *= FIX_2_053119869;
    t2 *= FIX_3_072711026;
    t3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223;
    z2 *= -FIX_2_562915447;
    z3 *= -FIX_1_961570560;
    z4 *= -FIX_0_390180644;
    z3 += z5;
    z4 += z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const int half = 1 << (shift - 1);
    out[0] = (tmp10 + t3 + half) >> shift;
    out[7] = (tmp10 - t3 + half) >> shift;
    out[1] = (tmp11 + t2 + half) >> shift;
    out[6] = (tmp11 - t2 + half) >> shift;
    out[2] = (tmp12 + t1 + half) >> shift;
    out[5] = (tmp12 - t1 + half) >> shift;
    out[3] = (tmp13 + t0 + half) >> shift;
    out[4] = (tmp13 - t0 + half) >> shift;
}

// grid (ceil(max blocks / 256), 3 * images): one block of a component per thread
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const Img* imgs, const uint16_t* quant, int num_quant) {
    const Img& im = imgs[blockIdx.y / 3];
    const int c = blockIdx.y % 3;
    const uint32_t blk = blockIdx.x * 256u + threadIdx.x;
    const int wb = im.wb[c];
    if (blk >= (uint32_t)wb * im.hb[c]) return;
    int qi = im.qt[c];
    qi = qi < 0 ? 0 : (qi >= num_quant ? num_quant - 1 : qi);
    const uint16_t* q = quant + (size_t)qi * 64;
    const int16_t* src = im.coef[c] + (size_t)blk * 64;
    int ws[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {   // dequantise, a row of coefficients per 16-byte load
        const int4 cv = *reinterpret_cast<const int4*>(src + r * 8);
        const int4 qv = *reinterpret_cast<const int4*>(q + r * 8);
        const int cw[4] = {cv.x, cv.y, cv.z, cv.w};
        const int qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[r * 8 + 2 * j] = (int)(int16_t)(cw[j] & 0xFFFF) * (int)(qw[j] & 0xFFFF);
            ws[r * 8 + 2 * j + 1] = (cw[j] >> 16) * (int)((uint32_t)qw[j] >> 16);
        }
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) {   // columns, PASS1_BITS kept: shift 13 - 2
        int in[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) in[y] = ws[y * 8 + x];
        idct8(in, o, 11);
#pragma unroll
        for (int y = 0; y < 8; ++y) ws[y * 8 + x] = o[y];
    }
    const int bx = (int)(blk % (uint32_t)wb), by = (int)(blk / (uint32_t)wb);
    uint8_t* dst = im.plane[c] + ((size_t)by * 8) * ((size_t)wb * 8) + (size_t)bx * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {   // rows: shift 13 + 2 + 3
        int o[8];
        idct8(ws + y * 8, o, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            int v = o[x] + 128;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            if (x < 4) lo |= (uint32_t)v << (8 * x);
            else hi |= (uint32_t)v << (8 * (x - 4));
        }
        *reinterpret_cast<uint2*>(dst + (size_t)y * wb * 8) = make_uint2(lo, hi);
    }
}

// one chroma sample at full resolution: libjpeg's upsamplers on the plane cropped to cw x ch
__device__ __forceinline__ int chroma_at(const uint8_t* pl, int stride, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return pl[(size_t)y * stride + x];
    const int i = x >> 1;
    if (cw <= 2) return pl[(size_t)(vs == 2 ? y >> 1 : y) * stride + i];   // replication, both ways
    if (vs == 1) {
        const uint8_t* row = pl + (size_t)y * stride;
        const int cur = row[i];
        if (x & 1) return i == cw - 1 ? cur : (3 * cur + row[i + 1] + 2) >> 2;
        return i == 0 ? cur : (3 * cur + row[i - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    int ny = (y & 1) ? cy + 1 : cy - 1;
    ny = ny < 0 ? 0 : (ny > ch - 1 ? ch - 1 : ny);
    const uint8_t* r0 = pl + (size_t)cy * stride;
    const uint8_t* r1 = pl + (size_t)ny * stride;
    const int cur = 3 * r0[i] + r1[i];
    if (x & 1) return i == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

// grid (ceil(max pixels / 256), images)
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const Img* imgs) {
    const Img& im = imgs[blockIdx.y];
    const uint32_t n = (uint32_t)im.h * im.w;
    const int cw = (im.w + im.hs - 1) / im.hs, ch = (im.h + im.vs - 1) / im.vs;
    for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
        const int y = (int)(p / (uint32_t)im.w), x = (int)(p % (uint32_t)im.w);
        const int Y = im.plane[0][(size_t)y * im.wb[0] * 8 + x];
        const int cb = chroma_at(im.plane[1], im.wb[1] * 8, cw, ch, im.hs, im.vs, x, y) - 128;
        const int cr = chroma_at(im.plane[2], im.wb[2] * 8, cw, ch, im.hs, im.vs, x, y) - 128;
        int r = Y + ((91881 * cr + 32768) >> 16);
        int g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        int b = Y + ((116130 * cb + 32768) >> 16);
        r = r < 0 ? 0 : (r > 255 ? 255 : r);
        g = g < 0 ? 0 : (g > 255 ? 255 : g);
        b = b < 0 ? 0 : (b > 255 ? 255 : b);
        uint8_t* o = im.out + (size_t)p * 3;
        o[0] = (uint8_t)r;
        o[1] = (uint8_t)g;
        o[2] = (uint8_t)b;
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Geometry {
    int hs, vs, mcux, mcuy, bpm;
    uint32_t nsub;
    size_t blocks[3];
    int wb[3], hb[3];
    size_t total_blocks;
};

const char* check_image(const md2_jpeg_image& im) {
    if (im.height < 1 || im.height > kMaxDim || im.width < 1 || im.width > kMaxDim)
        return "jpeg: height and width must be 1..8192";
    if (im.sampling != MD2_JPEG_444 && im.sampling != MD2_JPEG_422 && im.sampling != MD2_JPEG_420)
        return "jpeg: unsupported sampling class (4:4:4, 4:2:2 and 4:2:0 only)";
    if (im.stream_bytes > kMaxStream) return "jpeg: a stream above 2^28 bytes";
    if (im.stream_offset % 4) return "jpeg: stream_offset must be a multiple of 4";
    if (im.out_offset % 16) return "jpeg: out_offset must be a multiple of 16";
    return nullptr;
}

uint32_t stream_nsub(const md2_jpeg_image& im) {
    const uint32_t nsub = (uint32_t)(((uint64_t)im.stream_bytes * 8 + kSubBits - 1) / kSubBits);
    return nsub ? nsub : 1;
}

// an image's index: nsub 64-bit entry states, nsub 32-bit block counts, padded to 16 bytes
size_t index_size(uint32_t nsub) { return ((size_t)nsub * 12 + 15) & ~(size_t)15; }

Geometry geometry(const md2_jpeg_image& im) {
    Geometry g;
    g.hs = im.sampling == MD2_JPEG_444 ? 1 : 2;
    g.vs = im.sampling == MD2_JPEG_420 ? 2 : 1;
    g.mcux = (im.width + 8 * g.hs - 1) / (8 * g.hs);
    g.mcuy = (im.height + 8 * g.vs - 1) / (8 * g.vs);
    g.bpm = g.hs * g.vs + 2;
    for (int c = 0; c < 3; ++c) {
        g.wb[c] = g.mcux * (c ? 1 : g.hs);
        g.hb[c] = g.mcuy * (c ? 1 : g.vs);
        g.blocks[c] = (size_t)g.wb[c] * g.hb[c];
    }
    g.total_blocks = (size_t)g.mcux * g.mcuy * g.bpm;
    g.nsub = stream_nsub(im);
    return g;
}

// workspace: every image's coefficients (one memset), then samples, then the slot arrays
struct Layout {
    size_t coef_bytes, total;
};

const char* check_batch(const md2_jpeg_image* images, int n) {
    if (!images) return "jpeg: NULL images";
    if (n < 1) return "jpeg: a call needs at least one image";
    if (n > kMaxImages) return "jpeg: too many images (at most 4096 per call)";
    for (int i = 0; i < n; ++i)
        if (const char* msg = check_image(images[i])) return msg;
    return nullptr;
}

Layout layout(const md2_jpeg_image* images, int n) {
    Layout l;
    size_t coef = 0, rest = 0;
    for (int i = 0; i < n; ++i) {
        const Geometry g = geometry(images[i]);
        coef += align256(g.total_blocks * 64 * sizeof(int16_t));
        rest += align256(g.total_blocks * 64);
        rest += align256(((size_t)g.nsub + 1) * sizeof(unsigned long long));
        rest += align256(((size_t)g.nsub + 1) * sizeof(uint32_t));
        rest += align256((size_t)g.nsub * sizeof(uint32_t));
    }
    l.coef_bytes = coef;
    l.total = coef + rest;
    return l;
}

const char* check_ranges(const md2_jpeg_image* images, int n, int num_quant, int num_huff, uint64_t streams_bytes,
                         uint64_t out_bytes, bool frames) {
    if (num_quant < 1 || num_huff < 1 || num_quant > 256 || num_huff > 256)
        return "jpeg: the bank needs 1..256 quantisation and 1..256 Huffman tables";
    for (int i = 0; i < n; ++i) {
        const md2_jpeg_image& im = images[i];
        for (int c = 0; c < 3; ++c)
            if (im.quant[c] >= num_quant || im.dc[c] >= num_huff || im.ac[c] >= num_huff)
                return "jpeg: a table index is outside the bank";
        const uint64_t sb = ((uint64_t)im.stream_bytes + 3) / 4 * 4;   // whole words are fetched
        if (im.stream_offset > streams_bytes || sb > streams_bytes - im.stream_offset)
            return "jpeg: a stream reaches past streams_bytes";
        const uint64_t ob = (uint64_t)im.height * im.width * 3;
        if (frames && (im.out_offset > out_bytes || ob > out_bytes - im.out_offset))
            return "jpeg: a frame reaches past out_bytes";
    }
    return nullptr;
}

// every image's index lies, 16-byte aligned, inside a buffer of `bytes` bytes (`past`: what to say if not)
const char* check_index(const md2_jpeg_image* images, const uint64_t* index_offsets, int n, uint64_t bytes,
                        const char* past) {
    for (int i = 0; i < n; ++i) {
        if (index_offsets[i] % 16) return "jpeg: an index offset must be a multiple of 16";
        const uint64_t ib = index_size(stream_nsub(images[i]));
        if (index_offsets[i] > bytes || ib > bytes - index_offsets[i]) return past;
    }
    return nullptr;
}

}  // namespace

struct md2_jpeg_plan {
    int max_images = 0;
    size_t workspace_bytes = 0;
    char* workspace = nullptr;
    Img* dev_imgs = nullptr;      // kRing slots of max_images
    Img* host_imgs = nullptr;     // pinned, the same shape
    hipEvent_t staged[kRing] = {};
    int slot = 0;
};

// The launches of md2_jpeg_run (kRun), md2_jpeg_run_indexed (kRunIndexed: index_base is the
// streams buffer) and md2_jpeg_index (kIndex: index_base is the index buffer, out is NULL)
// for a batch that has passed their checks.
enum Mode { kRun, kRunIndexed, kIndex };

static int run_chain(Mode mode, md2_jpeg_plan* P, const uint8_t* streams, const md2_jpeg_image* images,
                     const uint64_t* index_offsets, int n, const md2_jpeg_bank* bank, uint8_t* out,
                     uint8_t* index_base, uint32_t* status, void* stream) {
    if (reinterpret_cast<uintptr_t>(streams) % 4)
        return md2_report_error(MD2_ERR_ARG, "jpeg: streams must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(bank->quant) % 16)
        return md2_report_error(MD2_ERR_ARG, "jpeg: bank.quant must be 16-byte aligned");
    if (n > P->max_images) return md2_report_error(MD2_ERR_ARG, "jpeg: more images than the plan was created for");
    const Layout l = layout(images, n);
    if (l.total > P->workspace_bytes)
        return md2_report_error(MD2_ERR_ARG, "jpeg: the batch needs more workspace than the plan owns");

    hipStream_t st = (hipStream_t)stream;
    const int r = P->slot;
    P->slot = (P->slot + 1) % kRing;
    if (hipEventSynchronize(P->staged[r]) != hipSuccess)
        return md2_report_error(MD2_ERR_HIP, "jpeg: waiting for a staging slot failed");
    Img* host = P->host_imgs + (size_t)r * P->max_images;
    Img* dev = P->dev_imgs + (size_t)r * P->max_images;
    size_t o_coef = 0, o_rest = l.coef_bytes, max_blocks = 0, max_pixels = 0;
    uint32_t max_nsub = 1;
    for (int i = 0; i < n; ++i) {
        const md2_jpeg_image& im = images[i];
        const Geometry g = geometry(im);
        Img& d = host[i];
        memset(&d, 0, sizeof(d));
        d.words = reinterpret_cast<const uint32_t*>(streams + im.stream_offset);
        d.nbytes = im.stream_bytes;
        d.h = im.height; d.w = im.width; d.hs = g.hs; d.vs = g.vs;
        d.mcux = g.mcux; d.mcuy = g.mcuy; d.bpm = g.bpm;
        d.total_blocks = (uint32_t)g.total_blocks;
        size_t oc = o_coef, op = o_rest;
        for (int c = 0; c < 3; ++c) {
            d.qt[c] = im.quant[c]; d.dct[c] = im.dc[c]; d.act[c] = im.ac[c];
            d.wb[c] = g.wb[c]; d.hb[c] = g.hb[c];
            d.coef[c] = reinterpret_cast<int16_t*>(P->workspace + oc);
            d.plane[c] = reinterpret_cast<uint8_t*>(P->workspace + op);
            oc += g.blocks[c] * 64 * sizeof(int16_t);
            op += g.blocks[c] * 64;
            if (g.blocks[c] > max_blocks) max_blocks = g.blocks[c];
        }
        o_coef += align256(g.total_blocks * 64 * sizeof(int16_t));
        o_rest += align256(g.total_blocks * 64);
        d.slots = reinterpret_cast<unsigned long long*>(P->workspace + o_rest);
        o_rest += align256(((size_t)g.nsub + 1) * sizeof(unsigned long long));
        d.dirty = reinterpret_cast<uint32_t*>(P->workspace + o_rest);
        o_rest += align256(((size_t)g.nsub + 1) * sizeof(uint32_t));
        d.counts = reinterpret_cast<uint32_t*>(P->workspace + o_rest);
        o_rest += align256((size_t)g.nsub * sizeof(uint32_t));
        d.nsub = g.nsub;
        d.out = out ? out + im.out_offset : nullptr;
        if (index_base) {
            d.ix_state = reinterpret_cast<unsigned long long*>(index_base + index_offsets[i]);
            d.ix_first = reinterpret_cast<uint32_t*>(d.ix_state + g.nsub);
        }
        if (g.nsub > max_nsub) max_nsub = g.nsub;
        d.status = status + i;
        const size_t px = (size_t)im.height * im.width;
        if (px > max_pixels) max_pixels = px;
    }
    if (hipMemcpyAsync(dev, host, (size_t)n * sizeof(Img), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipEventRecord(P->staged[r], st) != hipSuccess)
        return md2_report_error(MD2_ERR_HIP, "jpeg: staging the image table failed");
    const uint8_t* huff = static_cast<const uint8_t*>(bank->huff);
    const uint16_t* quant = static_cast<const uint16_t*>(bank->quant);
    if (mode == kIndex) {   // the synchronisation alone: no coefficient, sample or pixel is written
        hipLaunchKernelGGL(jpeg_entropy_kernel<true>, dim3(n), dim3(kThreads), 0, st, dev, huff, bank->num_huff);
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
    }
    if (hipMemsetAsync(P->workspace, 0, l.coef_bytes, st) != hipSuccess)
        return md2_report_error(MD2_ERR_HIP, "jpeg: hipMemsetAsync failed");
    if (mode == kRunIndexed) {
        // several workgroups of an image OR into its status word: cleared here, not by one of them
        if (hipMemsetAsync(status, 0, (size_t)n * sizeof(uint32_t), st) != hipSuccess)
            return md2_report_error(MD2_ERR_HIP, "jpeg: hipMemsetAsync failed");
        hipLaunchKernelGGL(jpeg_entropy_indexed_kernel, dim3((max_nsub + kIxThreads - 1) / kIxThreads, n),
                           dim3(kIxThreads), 0, st, dev, huff, bank->num_huff);
    } else {
        hipLaunchKernelGGL(jpeg_entropy_kernel<false>, dim3(n), dim3(kThreads), 0, st, dev, huff, bank->num_huff);
    }
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3, n), dim3(kThreads), 0, st, dev);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 255) / 256), 3 * n), dim3(256), 0, st, dev,
                       quant, bank->num_quant);
    size_t cb = (max_pixels + 255) / 256;
    if (cb > 4096) cb = 4096;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)cb, n), dim3(256), 0, st, dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

extern "C" {

size_t md2_jpeg_workspace_bytes(const md2_jpeg_image* images, int n) {
    if (const char* msg = check_batch(images, n)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return layout(images, n).total;
}

int md2_jpeg_check(const md2_jpeg_image* images, int n, int num_quant, int num_huff, uint64_t streams_bytes,
                   uint64_t out_bytes) {
    if (const char* msg = check_batch(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, num_quant, num_huff, streams_bytes, out_bytes, true))
        return md2_report_error(MD2_ERR_ARG, msg);
    return MD2_OK;
}

md2_jpeg_plan* md2_jpeg_plan_create(int max_images, size_t workspace_bytes) {
    if (max_images < 1 || max_images > kMaxImages)
        return md2_report_error(MD2_ERR_ARG, "jpeg: max_images must be 1..4096"), nullptr;
    if (workspace_bytes < 256) return md2_report_error(MD2_ERR_ARG, "jpeg: workspace_bytes below 256"), nullptr;
    auto* P = new (std::nothrow) md2_jpeg_plan();
    if (!P) return md2_report_error(MD2_ERR_ARG, "jpeg: out of host memory"), nullptr;
    P->max_images = max_images;
    P->workspace_bytes = align256(workspace_bytes);
    const size_t table = align256((size_t)kRing * max_images * sizeof(Img));
    bool ok = hipMalloc((void**)&P->workspace, P->workspace_bytes + table) == hipSuccess;
    if (ok) P->dev_imgs = reinterpret_cast<Img*>(P->workspace + P->workspace_bytes);
    ok = ok && hipHostMalloc((void**)&P->host_imgs, table, hipHostMallocDefault) == hipSuccess;
    for (int r = 0; ok && r < kRing; ++r)
        ok = hipEventCreateWithFlags(&P->staged[r], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        md2_jpeg_plan_destroy(P);
        return md2_report_error(MD2_ERR_HIP, "jpeg: workspace / pinned staging / events allocation failed"), nullptr;
    }
    return P;
}

void md2_jpeg_plan_destroy(md2_jpeg_plan* P) {
    if (!P) return;
    for (int r = 0; r < kRing; ++r)
        if (P->staged[r]) {
            (void)hipEventSynchronize(P->staged[r]);
            (void)hipEventDestroy(P->staged[r]);
        }
    if (P->host_imgs) (void)hipHostFree(P->host_imgs);
    if (P->workspace) (void)hipFree(P->workspace);
    delete P;
}

int md2_jpeg_run(md2_jpeg_plan* P, const uint8_t* streams, uint64_t streams_bytes, const md2_jpeg_image* images,
                 int n, const md2_jpeg_bank* bank, uint8_t* out, uint64_t out_bytes, uint32_t* status, void* stream) {
    if (!P || !streams || !images || !bank || !out || !status)
        return md2_report_error(MD2_ERR_ARG, "jpeg: plan/streams/images/bank/out/status is NULL");
    if (!bank->quant || !bank->huff) return md2_report_error(MD2_ERR_ARG, "jpeg: bank.quant/bank.huff is NULL");
    if (const char* msg = check_batch(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, bank->num_quant, bank->num_huff, streams_bytes, out_bytes, true))
        return md2_report_error(MD2_ERR_ARG, msg);
    return run_chain(kRun, P, streams, images, nullptr, n, bank, out, nullptr, status, stream);
}

size_t md2_jpeg_index_bytes(uint32_t stream_bytes) {
    md2_jpeg_image im = {};
    im.stream_bytes = stream_bytes;
    return index_size(stream_nsub(im));
}

int md2_jpeg_index(md2_jpeg_plan* P, const uint8_t* streams, uint64_t streams_bytes, const md2_jpeg_image* images,
                   const uint64_t* index_offsets, int n, const md2_jpeg_bank* bank, uint8_t* index,
                   uint64_t index_bytes, uint32_t* status, void* stream) {
    if (!P || !streams || !images || !index_offsets || !bank || !index || !status)
        return md2_report_error(MD2_ERR_ARG, "jpeg: plan/streams/images/index_offsets/bank/index/status is NULL");
    if (!bank->quant || !bank->huff) return md2_report_error(MD2_ERR_ARG, "jpeg: bank.quant/bank.huff is NULL");
    if (const char* msg = check_batch(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, bank->num_quant, bank->num_huff, streams_bytes, 0, false))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_index(images, index_offsets, n, index_bytes, "jpeg: an index reaches past index_bytes"))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (reinterpret_cast<uintptr_t>(index) % 16)
        return md2_report_error(MD2_ERR_ARG, "jpeg: index must be 16-byte aligned");
    return run_chain(kIndex, P, streams, images, index_offsets, n, bank, nullptr, index, status, stream);
}

int md2_jpeg_check_indexed(const md2_jpeg_image* images, const uint64_t* index_offsets, int n, int num_quant,
                           int num_huff, uint64_t streams_bytes, uint64_t out_bytes) {
    if (!images || !index_offsets) return md2_report_error(MD2_ERR_ARG, "jpeg: images/index_offsets is NULL");
    if (const char* msg = check_batch(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, num_quant, num_huff, streams_bytes, out_bytes, true))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg =
            check_index(images, index_offsets, n, streams_bytes, "jpeg: an index reaches past streams_bytes"))
        return md2_report_error(MD2_ERR_ARG, msg);
    return MD2_OK;
}

int md2_jpeg_run_indexed(md2_jpeg_plan* P, const uint8_t* streams, uint64_t streams_bytes,
                         const md2_jpeg_image* images, const uint64_t* index_offsets, int n,
                         const md2_jpeg_bank* bank, uint8_t* out, uint64_t out_bytes, uint32_t* status, void* stream) {
    if (!P || !streams || !images || !index_offsets || !bank || !out || !status)
        return md2_report_error(MD2_ERR_ARG, "jpeg: plan/streams/images/index_offsets/bank/out/status is NULL");
    if (!bank->quant || !bank->huff) return md2_report_error(MD2_ERR_ARG, "jpeg: bank.quant/bank.huff is NULL");
    if (const char* msg = check_batch(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, bank->num_quant, bank->num_huff, streams_bytes, out_bytes, true))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg =
            check_index(images, index_offsets, n, streams_bytes, "jpeg: an index reaches past streams_bytes"))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (reinterpret_cast<uintptr_t>(streams) % 16)
        return md2_report_error(MD2_ERR_ARG, "jpeg: streams must be 16-byte aligned when they carry indexes");
    return run_chain(kRunIndexed, P, streams, images, index_offsets, n, bank, out, const_cast<uint8_t*>(streams),
                     status, stream);
}

}  // extern "C"
