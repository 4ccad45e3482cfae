// jpegenc.hip — baseline JPEG encoding on gfx950: tight (h, w, 3) RGB frames of a batch ->
// the unstuffed entropy-coded segment of each, every byte what Pillow (libjpeg's default
// integer path: 16-bit fixed-point colour, box downsampling, jfdctint's islow transform, the
// standard Huffman tables) writes between its SOS header and EOI for the same frame, quality
// and sampling.  The other half of jpeg.hip; the host writes the file around the segment
// (monodepth2_amd/jpeg_ops.py, jpeg_file_bytes).
//
// md2_jpeg_encode (include/md2hot.h) is a fixed chain of launches for the whole batch, the
// image on grid.y, blocks in scan order (MCU by MCU: its luma blocks in raster order, Cb, Cr):
//
//   setup    one thread: the geometry of every image and where its arrays lie in the workspace
//   dct      one thread per block: colour conversion and downsampling on the fly from RGB
//            (clamped reads), forward DCT, quantisation -> 64 int16 in zigzag order
//   count    one thread per block: the bits of its codes.  The DC predecessor of a block is at
//            a computable address (the block before it in the MCU, or the same component's last
//            block of the MCU before), so nothing walks the scan
//   scan     one workgroup per image: exclusive scan of the bit counts (64-bit offsets), the
//            stream's length and the status word
//   zero     the bytes of every stream that fits its range
//   emit     one thread per block: its codes assembled into whole 32-bit words in registers; a
//            span's first and last word are shared with a neighbour and take an integer atomic
//            OR, the words between are plain stores
//
// A dummy block (one of the last MCU column or row beyond the luma plane's own blocks) has no
// samples: its AC coefficients are zero and its DC is the DC of the block before it in the MCU,
// so `dct` stores zeros for it and whoever needs its DC walks back to the last real block.
//
// Integer arithmetic only and no float atomics: two runs are bit-equal.  Nothing is written
// outside an image's output range: a stream that does not fit writes nothing at all.

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

namespace {

constexpr int kThreads = 256;         // dct, count, zero, emit
constexpr int kScanThreads = 1024;
constexpr int kMaxImages = 4096;      // per call
constexpr int kMaxDim = 8192;
constexpr int kBlockBytes = 208;      // a block is at most 20 + 63 * 26 = 1658 bits
constexpr int kSmpStride = 17;        // dwords per thread of the sample staging: 64 bytes + 1 dword, no bank conflicts
constexpr int kZeroBlocks = 512;      // grid.x of the zero kernel (grid-stride)

constexpr unsigned char kZigzag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU-T T.81 Annex K, tables K.3 to K.6: code counts by length, then the symbols.
constexpr unsigned char kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                          {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                          {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr unsigned char kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// symbol -> length << 16 | code, the canonical codes of the tables above, made by the compiler
struct Codes {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

constexpr Codes make_codes() {
    Codes c = {};
    for (int t = 0; t < 2; ++t) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kDcBits[t][len - 1]; ++i) c.dc[t][k++] = (uint32_t)len << 16 | code++;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kAcBits[t][len - 1]; ++i) c.ac[t][kAcVals[t][k++]] = (uint32_t)len << 16 | code++;
            code <<= 1;
        }
    }
    return c;
}

__device__ const Codes kCodes = make_codes();
constexpr int kCodeWords = sizeof(Codes) / sizeof(uint32_t);

struct Geometry {
    int hs, vs;               // luma sampling factors (chroma is 1 x 1)
    int mcux, mcuy, bpm;      // MCUs across and down, blocks per MCU
    int wb0, hb0;             // the luma plane's own blocks
    uint32_t total_blocks;    // of the scan, dummy blocks included
};

__host__ __device__ inline Geometry geometry(int h, int w, int sampling) {
    Geometry g;
    g.hs = sampling == MD2_JPEG_444 ? 1 : 2;
    g.vs = sampling == MD2_JPEG_420 ? 2 : 1;
    g.mcux = (w + 8 * g.hs - 1) / (8 * g.hs);
    g.mcuy = (h + 8 * g.vs - 1) / (8 * g.vs);
    g.bpm = g.hs * g.vs + 2;
    g.wb0 = (w + 7) / 8;
    g.hb0 = (h + 7) / 8;
    g.total_blocks = (uint32_t)g.mcux * (uint32_t)g.mcuy * (uint32_t)g.bpm;   // at most 3 * 2^20
    return g;
}

__host__ __device__ inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Img {                  // one image of the batch, in the workspace's table
    const uint8_t* rgb;
    uint32_t* out;            // the image's output range, 16-byte aligned
    uint32_t cap;             // bytes
    int h, w;
    Geometry g;
    int ql, qc;               // quantisation tables of the bank
    int16_t* coef;            // total_blocks x 64, zigzag order, scan order
    uint32_t* bits;           // total_blocks
    unsigned long long* offs; // total_blocks: the bit each block starts at
};

__host__ __device__ inline size_t table_bytes(int n) { return align256((size_t)n * sizeof(Img)); }
__host__ __device__ inline size_t image_bytes(uint32_t total_blocks) {
    return align256((size_t)total_blocks * 64 * sizeof(int16_t)) + align256((size_t)total_blocks * sizeof(uint32_t)) +
           align256((size_t)total_blocks * sizeof(unsigned long long));
}

// ------------------------------------------------------------------ setup
__global__ void jpegenc_setup_kernel(const md2_jpegenc_image* __restrict__ images, int n, const uint8_t* in,
                                     uint8_t* out, char* workspace) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Img* table = reinterpret_cast<Img*>(workspace);
    size_t pos = table_bytes(n);
    for (int i = 0; i < n; ++i) {
        const md2_jpegenc_image im = images[i];
        Img d;
        d.rgb = in + im.in_offset;
        d.out = reinterpret_cast<uint32_t*>(out + im.out_offset);
        d.cap = im.out_capacity;
        d.h = im.height;
        d.w = im.width;
        d.g = geometry(im.height, im.width, im.sampling);
        d.ql = im.quant[0];
        d.qc = im.quant[1];
        const size_t tb = d.g.total_blocks;
        d.coef = reinterpret_cast<int16_t*>(workspace + pos);
        pos += align256(tb * 64 * sizeof(int16_t));
        d.bits = reinterpret_cast<uint32_t*>(workspace + pos);
        pos += align256(tb * sizeof(uint32_t));
        d.offs = reinterpret_cast<unsigned long long*>(workspace + pos);
        pos += align256(tb * sizeof(unsigned long long));
        table[i] = d;
    }
}

// block g of the scan: component, position in its component plane, dummy or not
struct BlockPos {
    uint32_t m;
    int b, c, by, bx;
    bool dummy;
};

__device__ __forceinline__ BlockPos block_pos(const Geometry& g, uint32_t blk) {
    BlockPos p;
    p.m = blk / (uint32_t)g.bpm;
    p.b = (int)(blk - p.m * (uint32_t)g.bpm);
    const int my = (int)(p.m / (uint32_t)g.mcux), mx = (int)(p.m - (uint32_t)my * (uint32_t)g.mcux);
    const int ny = g.hs * g.vs;
    if (p.b < ny) {
        p.c = 0;
        p.by = my * g.vs + p.b / g.hs;
        p.bx = mx * g.hs + p.b % g.hs;
        p.dummy = p.by >= g.hb0 || p.bx >= g.wb0;
    } else {
        p.c = p.b - ny + 1;
        p.by = my;
        p.bx = mx;
        p.dummy = false;
    }
    return p;
}

// ------------------------------------------------------------------ dct
// jfdctint's eight-point pass.  kRow: outputs 0 and 4 scaled up by 2 bits, the others descaled
// by 11; else (columns) 2 and 15.
template <bool kRow>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int n = kRow ? 11 : 15;
    constexpr int half = 1 << (n - 1);
    const int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6;
    const int tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (kRow) {
        d0 = (tmp10 + tmp11) * 4;
        d4 = (tmp10 - tmp11) * 4;
    } else {
        d0 = (tmp10 + tmp11 + 2) >> 2;
        d4 = (tmp10 - tmp11 + 2) >> 2;
    }
    int z1 = (tmp12 + tmp13) * 4433;
    d2 = (z1 + tmp13 * 6270 + half) >> n;
    d6 = (z1 - tmp12 * 15137 + half) >> n;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d7 = (t4 + z1 + z3 + half) >> n;
    d5 = (t5 + z2 + z4 + half) >> n;
    d3 = (t6 + z2 + z3 + half) >> n;
    d1 = (t7 + z1 + z4 + half) >> n;
}

__global__ __launch_bounds__(kThreads) void jpegenc_dct_kernel(const char* workspace,
                                                               const uint16_t* __restrict__ quant) {
    __shared__ uint32_t smp[kThreads * kSmpStride];
    __shared__ uint32_t qstep[128];    // 8 q: luma, then chroma
    __shared__ uint32_t qmagic[128];   // ceil(2^32 / (8 q)): exact quotients for numerators below 2^21
    const Img& im = reinterpret_cast<const Img*>(workspace)[blockIdx.y];
    const Geometry g = im.g;
    if (blockIdx.x * kThreads >= g.total_blocks) return;   // the whole workgroup
    const int tid = threadIdx.x;
    if (tid < 128) {
        const uint32_t d = 8u * quant[(size_t)(tid < 64 ? im.ql : im.qc) * 64 + (tid & 63)];
        qstep[tid] = d;
        qmagic[tid] = d ? (uint32_t)((0x100000000ull + d - 1) / d) : 0u;
    }
    const uint32_t blk = blockIdx.x * kThreads + tid;
    const bool live = blk < g.total_blocks;
    BlockPos p = {};
    if (live) p = block_pos(g, blk);
    uint8_t* mine = reinterpret_cast<uint8_t*>(smp + tid * kSmpStride);
    if (live && !p.dummy) {
        const int h = im.h, w = im.w;
        const int chs = p.c == 0 ? 1 : g.hs, cvs = p.c == 0 ? 1 : g.vs;
        const int ch = (h + cvs - 1) / cvs;
        // 16-bit fixed point, libjpeg's rgb_ycc tables: Y rounds at a half, Cb and Cr just below
        const int kr = p.c == 0 ? 19595 : p.c == 1 ? -11059 : 32768;
        const int kg = p.c == 0 ? 38470 : p.c == 1 ? -21709 : -27439;
        const int kb = p.c == 0 ? 7471 : p.c == 1 ? 32768 : -5329;
        const int ka = p.c == 0 ? 32768 : (128 << 16) + 32767;
        const int shift = (chs == 2) + (cvs == 2);
        for (int r = 0; r < 8; ++r) {
            int cy = p.by * 8 + r;
            if (cy > ch - 1) cy = ch - 1;          // the downsampled last row is repeated
            for (int col = 0; col < 8; ++col) {
                const int cx = p.bx * 8 + col;
                int sum = 0;
                for (int dy = 0; dy < cvs; ++dy) {
                    int y = cy * cvs + dy;
                    if (y > h - 1) y = h - 1;      // rows extended to a multiple of the factor
                    const uint8_t* row = im.rgb + (size_t)y * w * 3;
                    for (int dx = 0; dx < chs; ++dx) {
                        int x = cx * chs + dx;
                        if (x > w - 1) x = w - 1;  // the last pixel repeated before downsampling
                        const uint8_t* px = row + (size_t)x * 3;
                        sum += (kr * px[0] + kg * px[1] + kb * px[2] + ka) >> 16;
                    }
                }
                const int bias = shift == 0 ? 0 : shift == 1 ? (cx & 1) : 1 + (cx & 1);
                mine[r * 8 + col] = (uint8_t)((sum + bias) >> shift);
            }
        }
    }
    __syncthreads();   // the tables; every thread reads back only its own samples
    if (!live) return;
    uint4* dst = reinterpret_cast<uint4*>(im.coef + (size_t)blk * 64);
    if (p.dummy) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = make_uint4(0, 0, 0, 0);
        return;
    }
    int ws[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint32_t lo = smp[tid * kSmpStride + 2 * r], hi = smp[tid * kSmpStride + 2 * r + 1];
        ws[r * 8 + 0] = (int)(lo & 255) - 128;
        ws[r * 8 + 1] = (int)(lo >> 8 & 255) - 128;
        ws[r * 8 + 2] = (int)(lo >> 16 & 255) - 128;
        ws[r * 8 + 3] = (int)(lo >> 24) - 128;
        ws[r * 8 + 4] = (int)(hi & 255) - 128;
        ws[r * 8 + 5] = (int)(hi >> 8 & 255) - 128;
        ws[r * 8 + 6] = (int)(hi >> 16 & 255) - 128;
        ws[r * 8 + 7] = (int)(hi >> 24) - 128;
        fdct8<true>(ws[r * 8 + 0], ws[r * 8 + 1], ws[r * 8 + 2], ws[r * 8 + 3], ws[r * 8 + 4], ws[r * 8 + 5],
                    ws[r * 8 + 6], ws[r * 8 + 7]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)
        fdct8<false>(ws[c], ws[8 + c], ws[16 + c], ws[24 + c], ws[32 + c], ws[40 + c], ws[48 + c], ws[56 + c]);
    const int qbase = p.c == 0 ? 0 : 64;
    uint32_t packed[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int nat = kZigzag[k];
        const int v = ws[nat];
        const uint32_t d = qstep[qbase + nat];
        const uint32_t mag = __umulhi((uint32_t)(v < 0 ? -v : v) + (d >> 1), qmagic[qbase + nat]);
        const uint32_t q = (uint32_t)(v < 0 ? -(int)mag : (int)mag) & 0xFFFFu;
        if (k & 1)
            packed[k >> 1] |= q << 16;
        else
            packed[k >> 1] = q;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        dst[i] = make_uint4(packed[4 * i], packed[4 * i + 1], packed[4 * i + 2], packed[4 * i + 3]);
}

// ------------------------------------------------------------------ codes
// The DC of block (m, b): a dummy block has the DC of the last real block before it in the MCU
// (block 0 of an MCU is always real).
__device__ __forceinline__ int dc_value(const Img& im, uint32_t m, int b) {
    const Geometry& g = im.g;
    if (b < g.hs * g.vs) {
        const int my = (int)(m / (uint32_t)g.mcux), mx = (int)(m - (uint32_t)my * (uint32_t)g.mcux);
        while (b > 0 && (my * g.vs + b / g.hs >= g.hb0 || mx * g.hs + b % g.hs >= g.wb0)) --b;
    }
    return im.coef[((size_t)m * g.bpm + b) * 64];
}

__device__ __forceinline__ int magnitude_bits(int v) {
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return 32 - __clz(a);   // 0 for 0
}

// Every code of block blk handed to sink.put(code, length) in stream order.  codes: LDS copy
// of kCodes.
template <class Sink>
__device__ __forceinline__ void code_block(const Img& im, uint32_t blk, const uint32_t* codes, Sink& sink) {
    const Geometry& g = im.g;
    const uint32_t m = blk / (uint32_t)g.bpm;
    const int b = (int)(blk - m * (uint32_t)g.bpm);
    const int ny = g.hs * g.vs;
    const int t = b < ny ? 0 : 1;
    int pred = 0;
    if (b < ny) {
        if (b > 0)
            pred = dc_value(im, m, b - 1);
        else if (m > 0)
            pred = dc_value(im, m - 1, ny - 1);
    } else if (m > 0) {
        pred = dc_value(im, m - 1, b);
    }
    const int diff = dc_value(im, m, b) - pred;
    int nb = magnitude_bits(diff);
    uint32_t e = codes[t * 16 + nb];
    sink.put(e & 0xFFFFu, (int)(e >> 16));
    if (nb) sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u), nb);
    const uint32_t* ac = codes + 32 + t * 256;
    const uint4* src = reinterpret_cast<const uint4*>(im.coef + (size_t)blk * 64);
    int run = 0;
    for (int i = 0; i < 8; ++i) {
        const uint4 q = src[i];
        const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (i == 0 && j == 0) continue;   // the DC (a dummy block's AC are stored as zeros)
            const int v = (int)(int16_t)(wds[j >> 1] >> (16 * (j & 1)));
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                e = ac[0xF0];
                sink.put(e & 0xFFFFu, (int)(e >> 16));
                run -= 16;
            }
            nb = magnitude_bits(v);
            e = ac[(run << 4 | nb) & 255];
            sink.put(e & 0xFFFFu, (int)(e >> 16));
            sink.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u), nb);
            run = 0;
        }
    }
    if (run) {
        e = ac[0];
        sink.put(e & 0xFFFFu, (int)(e >> 16));
    }
}

__device__ __forceinline__ void load_codes(uint32_t* codes) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&kCodes);
    for (int i = threadIdx.x; i < kCodeWords; i += blockDim.x) codes[i] = src[i];
    __syncthreads();
}

struct CountSink {
    uint32_t n = 0;
    __device__ __forceinline__ void put(uint32_t, int len) { n += (uint32_t)len; }
};

__global__ __launch_bounds__(kThreads) void jpegenc_count_kernel(const char* workspace) {
    __shared__ uint32_t codes[kCodeWords];
    const Img& im = reinterpret_cast<const Img*>(workspace)[blockIdx.y];
    if (blockIdx.x * kThreads >= im.g.total_blocks) return;
    load_codes(codes);
    const uint32_t blk = blockIdx.x * kThreads + threadIdx.x;
    if (blk >= im.g.total_blocks) return;
    CountSink sink;
    code_block(im, blk, codes, sink);
    im.bits[blk] = sink.n;
}

// ------------------------------------------------------------------ scan
__global__ __launch_bounds__(kScanThreads) void jpegenc_scan_kernel(const char* workspace,
                                                                    uint32_t* __restrict__ stream_bytes,
                                                                    uint32_t* __restrict__ status) {
    __shared__ uint32_t wave_sum[kScanThreads / 64];
    const Img& im = reinterpret_cast<const Img*>(workspace)[blockIdx.x];
    const uint32_t tb = im.g.total_blocks;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < tb; base += kScanThreads) {
        const uint32_t i = base + tid;
        const uint32_t v = i < tb ? im.bits[i] : 0u;
        uint32_t x = v;   // inclusive over the wave: at most 64 * 1658
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wave_sum[wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kScanThreads / 64; ++k) {
            const uint32_t s = wave_sum[k];
            if (k < wave) before += s;
            total += s;
        }
        if (i < tb) im.offs[i] = carry + before + (x - v);
        carry += total;
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned long long bytes = (carry + 7) >> 3;   // at most 3 * 2^20 * 208
        stream_bytes[blockIdx.x] = (uint32_t)bytes;
        status[blockIdx.x] = bytes > im.cap ? MD2_JPEGENC_ST_SPACE : 0u;
    }
}

// ------------------------------------------------------------------ zero, emit
__global__ __launch_bounds__(kThreads) void jpegenc_zero_kernel(const char* workspace,
                                                                const uint32_t* __restrict__ stream_bytes) {
    const Img& im = reinterpret_cast<const Img*>(workspace)[blockIdx.y];
    const uint32_t bytes = stream_bytes[blockIdx.y];
    if (bytes > im.cap) return;   // does not fit: nothing of the range is written
    const uint32_t words = (bytes + 3) / 4;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < words; i += gridDim.x * kThreads) {
        if ((unsigned long long)i * 4 + 4 <= im.cap) {
            im.out[i] = 0u;
        } else {                  // the range ends inside this word
            uint8_t* p = reinterpret_cast<uint8_t*>(im.out + i);
            for (uint32_t k = 0; (unsigned long long)i * 4 + k < im.cap; ++k) p[k] = 0;
        }
    }
}

// Big-endian bit packer into the zeroed range: whole words from a 64-bit register window.  A
// span's first word (bits of the block before may share it) and its last take an atomic OR;
// every word between is this block's alone.  Bits outside the stream are OR-ed as zeros.
struct EmitSink {
    uint32_t* words;
    unsigned long long acc;
    int fill;
    bool first;
    __device__ __forceinline__ void put(uint32_t code, int len) {
        acc = acc << len | code;   // fill < 32 and len <= 16
        fill += len;
        if (fill >= 32) {
            fill -= 32;
            const uint32_t w = __builtin_bswap32((uint32_t)(acc >> fill));
            if (first)
                atomicOr(words, w);
            else
                *words = w;
            first = false;
            ++words;
            acc &= (1ull << fill) - 1ull;
        }
    }
    __device__ __forceinline__ void finish() {
        if (fill > 0) atomicOr(words, __builtin_bswap32((uint32_t)(acc << (32 - fill))));
    }
};

__global__ __launch_bounds__(kThreads) void jpegenc_emit_kernel(const char* workspace,
                                                                const uint32_t* __restrict__ stream_bytes) {
    __shared__ uint32_t codes[kCodeWords];
    const Img& im = reinterpret_cast<const Img*>(workspace)[blockIdx.y];
    const uint32_t tb = im.g.total_blocks;
    if (blockIdx.x * kThreads >= tb) return;
    const uint32_t bytes = stream_bytes[blockIdx.y];
    if (bytes > im.cap) return;   // does not fit: nothing of the range is written
    load_codes(codes);
    const uint32_t blk = blockIdx.x * kThreads + threadIdx.x;
    if (blk >= tb) return;
    const unsigned long long off = im.offs[blk];
    EmitSink sink;
    sink.words = im.out + (off >> 5);
    sink.acc = 0;
    sink.fill = (int)(off & 31);
    sink.first = true;
    code_block(im, blk, codes, sink);
    if (blk == tb - 1) {          // the last byte is filled with 1-bits
        const int pad = (int)((8u - ((uint32_t)(off + im.bits[blk]) & 7u)) & 7u);
        if (pad) sink.put((1u << pad) - 1u, pad);
    }
    sink.finish();
}

const char* check_images(const md2_jpegenc_image* images, int n) {
    if (!images) return "jpeg encode: images is NULL";
    if (n < 1 || n > kMaxImages) return "jpeg encode: n must be 1..4096";
    for (int i = 0; i < n; ++i) {
        const md2_jpegenc_image& im = images[i];
        if (im.height < 1 || im.height > kMaxDim || im.width < 1 || im.width > kMaxDim)
            return "jpeg encode: height and width must be 1..8192";
        if (im.sampling != MD2_JPEG_444 && im.sampling != MD2_JPEG_422 && im.sampling != MD2_JPEG_420)
            return "jpeg encode: unknown sampling class";
    }
    return nullptr;
}

size_t workspace_need(const md2_jpegenc_image* images, int n) {
    size_t total = table_bytes(n);
    for (int i = 0; i < n; ++i)
        total += image_bytes(geometry(images[i].height, images[i].width, images[i].sampling).total_blocks);
    return total;
}

const char* check_ranges(const md2_jpegenc_image* images, int n, int num_quant, uint64_t in_bytes,
                         uint64_t out_bytes) {
    if (num_quant < 1 || num_quant > 256) return "jpeg encode: num_quant must be 1..256";
    for (int i = 0; i < n; ++i) {
        const md2_jpegenc_image& im = images[i];
        const uint64_t ib = (uint64_t)im.height * im.width * 3;
        if (im.in_offset > in_bytes || ib > in_bytes - im.in_offset) return "jpeg encode: a frame reaches past in_bytes";
        if (im.out_offset % 16) return "jpeg encode: out_offset must be a multiple of 16";
        const uint64_t ob = ((uint64_t)im.out_capacity + 3) / 4 * 4;   // whole words take the atomic OR
        const uint64_t room = (out_bytes + 3) / 4 * 4;
        if (im.out_offset > out_bytes || im.out_capacity > out_bytes - im.out_offset || ob > room - im.out_offset)
            return "jpeg encode: an output range reaches past out_bytes";
        if (im.quant[0] >= num_quant || im.quant[1] >= num_quant)
            return "jpeg encode: a table index is outside the bank";
    }
    return nullptr;
}

}  // namespace

extern "C" {

size_t md2_jpeg_encode_bound(int height, int width, int sampling) {
    md2_jpegenc_image im = {};
    im.height = height;
    im.width = width;
    im.sampling = sampling;
    if (const char* msg = check_images(&im, 1)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return (size_t)geometry(height, width, sampling).total_blocks * kBlockBytes;
}

size_t md2_jpeg_encode_workspace_bytes(const md2_jpegenc_image* images, int n) {
    if (const char* msg = check_images(images, n)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return workspace_need(images, n);
}

int md2_jpeg_encode_check(const md2_jpegenc_image* images, int n, int num_quant, uint64_t in_bytes,
                          uint64_t out_bytes) {
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, num_quant, in_bytes, out_bytes))
        return md2_report_error(MD2_ERR_ARG, msg);
    return MD2_OK;
}

int md2_jpeg_encode(const uint8_t* in, uint64_t in_bytes, const md2_jpegenc_image* images,
                    const md2_jpegenc_image* dev_images, int n, const uint16_t* quant, int num_quant, uint8_t* out,
                    uint64_t out_bytes, void* workspace, size_t workspace_bytes, uint32_t* stream_bytes,
                    uint32_t* status, void* stream) {
    if (!in || !images || !dev_images || !quant || !out || !workspace || !stream_bytes || !status)
        return md2_report_error(MD2_ERR_ARG,
                                "jpeg encode: in/images/dev_images/quant/out/workspace/stream_bytes/status is NULL");
    if (const char* msg = check_images(images, n)) return md2_report_error(MD2_ERR_ARG, msg);
    if (const char* msg = check_ranges(images, n, num_quant, in_bytes, out_bytes))
        return md2_report_error(MD2_ERR_ARG, msg);
    if (reinterpret_cast<uintptr_t>(out) % 16 || reinterpret_cast<uintptr_t>(workspace) % 256 ||
        reinterpret_cast<uintptr_t>(dev_images) % 8 || reinterpret_cast<uintptr_t>(quant) % 2)
        return md2_report_error(MD2_ERR_ARG,
                                "jpeg encode: out must be 16-byte, workspace 256-byte, dev_images 8-byte aligned");
    if (workspace_need(images, n) > workspace_bytes)
        return md2_report_error(MD2_ERR_ARG, "jpeg encode: the batch needs more workspace than workspace_bytes");
    uint32_t max_blocks = 1;
    for (int i = 0; i < n; ++i) {
        const uint32_t tb = geometry(images[i].height, images[i].width, images[i].sampling).total_blocks;
        if (tb > max_blocks) max_blocks = tb;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const dim3 per_block((max_blocks + kThreads - 1) / kThreads, n);
    unsigned zb = (unsigned)(((size_t)max_blocks * kBlockBytes / 4 + kThreads - 1) / kThreads);
    if (zb > kZeroBlocks) zb = kZeroBlocks;
    hipLaunchKernelGGL(jpegenc_setup_kernel, dim3(1), dim3(64), 0, st, dev_images, n, in, out, ws);
    hipLaunchKernelGGL(jpegenc_dct_kernel, per_block, dim3(kThreads), 0, st, ws, quant);
    hipLaunchKernelGGL(jpegenc_count_kernel, per_block, dim3(kThreads), 0, st, ws);
    hipLaunchKernelGGL(jpegenc_scan_kernel, dim3(n), dim3(kScanThreads), 0, st, ws, stream_bytes, status);
    hipLaunchKernelGGL(jpegenc_zero_kernel, dim3(zb, n), dim3(kThreads), 0, st, ws, stream_bytes);
    hipLaunchKernelGGL(jpegenc_emit_kernel, per_block, dim3(kThreads), 0, st, ws, stream_bytes);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
