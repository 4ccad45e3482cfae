// viz.hip — single-image depth inference's picture (the tail of test_simple.py) on gfx950:
// a batch of scale-0 disparities -> the magma-coloured uint8 images the reference saves.
//
// Reference: test_simple.py:136-155 resizes the disparity to the original image size with
// F.interpolate(bilinear, align_corners=False), then on the host, one image at a time, takes
// np.percentile(., 95) and .min(), normalises with matplotlib's Normalize, looks the values
// up in the `magma` colormap and converts to uint8.  Here (md2_disp_colorize,
// include/md2hot.h) a batch is a fixed chain of launches, the image on grid.y:
//
//   memset        the radix histograms
//   resize        one thread per output pixel (strided): bilinear sample -> workspace plane
//                 (and `resized`); per block the minimum key and a NaN flag through a fixed
//                 LDS tree; histogram of the top byte of the order-preserving keys
//   select x4     per (image, rank): the bin holding the rank-th key, the rank reduced
//   hist   x3     histogram of the next byte of the keys that match the prefix so far
//   finalise      one block per image: block partials folded in a fixed tree -> vmin, the
//                 NaN flag; vmax from the two selected order statistics (numpy's `linear`)
//   colourise     normalise, look up, pack: four pixels (12 bytes) per thread
//
// Arithmetic.  Every product and sum is a separately rounded operation in the written
// order (no contraction), so tests/viz_case.py restates the operator in numpy bit for bit.
// The resize and the percentile are fp32 throughout, as torch and numpy evaluate them on
// fp32 arrays; the normalisation's subtraction and division are fp64 operations rounded
// back to fp32 each (matplotlib divides the fp32 array by the fp64 range).
//
// A float's order-preserving key: the bits with the sign flipped when positive, all bits
// flipped when negative, so keys order as the values do (-0 below +0) and the k-th smallest
// value is the k-th smallest key: four 8-bit passes give the exact order statistic.  The
// two ranks numpy interpolates between are known on the host (they depend on the element
// count and the percentile only).  Histograms are integer atomics (they commute) and the
// minimum is an integer minimum of keys; no float atomic anywhere: bitwise repeatable.
//
// The resized map stays in the workspace (4 bytes a pixel written once, read by the three
// histogram passes and the colouriser) instead of being resampled four times: DESIGN §6e.

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 256;
constexpr int kRanks = 2;                 // the order statistics a[lo], a[lo + 1]
constexpr int kPasses = 4;
constexpr int kMaxBlocksPerImage = 256;   // also the width of the finalise tree
constexpr int kPixelsPerThread = 4;
constexpr int kMaxBatch = 65535;          // images are grid.y
constexpr int kMaxPixels = 1 << 24;       // f32(n - 1) must be exact
constexpr unsigned kNan = 0x7FC00000u;

// matplotlib's `magma`, entry i of its 256-entry table as (uint8)(channel * 255), packed
// R | G << 8 | B << 16 (tests/golden/viz/make_viz_golden.py prints it; tests/test_viz_abi.py
// pins it to the golden and to the installed matplotlib)
__device__ const unsigned kMagma[256] = {
    0x030000, 0x040000, 0x060000, 0x070001, 0x090101, 0x0b0101, 0x0d0202, 0x0f0202,
    0x110303, 0x130304, 0x150404, 0x170405, 0x190506, 0x1b0507, 0x1d0608, 0x1f0709,
    0x22070a, 0x24080b, 0x26090c, 0x280a0d, 0x2a0a0e, 0x2c0b0f, 0x2f0c10, 0x310c11,
    0x330d12, 0x350d14, 0x380e15, 0x3a0e16, 0x3c0f17, 0x3f0f18, 0x41101a, 0x44101b,
    0x46101c, 0x49101e, 0x4b111f, 0x4d1120, 0x501122, 0x521123, 0x551125, 0x571126,
    0x591128, 0x5c112a, 0x5e112b, 0x60102d, 0x62102f, 0x651030, 0x671032, 0x681034,
    0x6a0f35, 0x6c0f37, 0x6e0f39, 0x6f0f3b, 0x710f3c, 0x720f3e, 0x730f40, 0x740f42,
    0x750f43, 0x760f45, 0x770f47, 0x781048, 0x79104a, 0x79104b, 0x7a114d, 0x7b114f,
    0x7b1250, 0x7c1252, 0x7c1353, 0x7d1355, 0x7d1457, 0x7e1558, 0x7e155a, 0x7e165b,
    0x7e175d, 0x7f175e, 0x7f1860, 0x7f1861, 0x7f1963, 0x801a65, 0x801a66, 0x801b68,
    0x801c69, 0x801c6b, 0x801d6c, 0x811e6e, 0x811e6f, 0x811f71, 0x811f73, 0x812074,
    0x812176, 0x812177, 0x812279, 0x81227a, 0x81237c, 0x81247e, 0x81247f, 0x812581,
    0x812582, 0x812684, 0x812685, 0x812787, 0x812889, 0x81288a, 0x80298c, 0x80298d,
    0x802a8f, 0x802a91, 0x802b92, 0x802b94, 0x802c95, 0x7f2c97, 0x7f2d99, 0x7f2d9a,
    0x7f2e9c, 0x7e2e9e, 0x7e2f9f, 0x7e2fa1, 0x7e30a3, 0x7d30a4, 0x7d31a6, 0x7d31a7,
    0x7c32a9, 0x7c33ab, 0x7b33ac, 0x7b34ae, 0x7b34b0, 0x7a35b1, 0x7a35b3, 0x7936b5,
    0x7936b6, 0x7837b8, 0x7837b9, 0x7738bb, 0x7739bd, 0x7639be, 0x753ac0, 0x753ac2,
    0x743bc3, 0x743cc5, 0x733cc6, 0x723dc8, 0x723eca, 0x713ecb, 0x703fcd, 0x7040ce,
    0x6f41d0, 0x6e42d1, 0x6d42d3, 0x6d43d4, 0x6c44d6, 0x6b45d7, 0x6a46d9, 0x6947da,
    0x6948dc, 0x6849dd, 0x674ade, 0x664be0, 0x664ce1, 0x654de2, 0x644ee4, 0x6350e5,
    0x6251e6, 0x6252e7, 0x6154e8, 0x6055ea, 0x6056eb, 0x5f58ec, 0x5f59ed, 0x5e5bee,
    0x5d5dee, 0x5d5eef, 0x5d60f0, 0x5c61f1, 0x5c63f2, 0x5c65f3, 0x5b67f3, 0x5b68f4,
    0x5b6af5, 0x5b6cf5, 0x5b6ef6, 0x5b70f6, 0x5b71f7, 0x5c73f7, 0x5c75f8, 0x5c77f8,
    0x5c79f9, 0x5d7bf9, 0x5d7df9, 0x5e7ffa, 0x5e80fa, 0x5f82fa, 0x6084fb, 0x6086fb,
    0x6188fb, 0x628afb, 0x638cfc, 0x638efc, 0x6490fc, 0x6592fc, 0x6693fc, 0x6795fd,
    0x6897fd, 0x6999fd, 0x6a9bfd, 0x6b9dfd, 0x6c9ffd, 0x6ea1fd, 0x6fa2fd, 0x70a4fd,
    0x71a6fe, 0x73a8fe, 0x74aafe, 0x75acfe, 0x76aefe, 0x78affe, 0x79b1fe, 0x7bb3fe,
    0x7cb5fe, 0x7db7fe, 0x7fb9fe, 0x80bbfe, 0x82bcfe, 0x83befe, 0x85c0fe, 0x86c2fe,
    0x88c4fe, 0x89c6fe, 0x8bc7fe, 0x8dc9fe, 0x8ecbfe, 0x90cdfd, 0x92cffd, 0x93d1fd,
    0x95d2fd, 0x97d4fd, 0x98d6fd, 0x9ad8fd, 0x9cdafd, 0x9ddcfd, 0x9fddfd, 0xa1dffd,
    0xa3e1fd, 0xa5e3fc, 0xa6e5fc, 0xa8e6fc, 0xaae8fc, 0xaceafc, 0xaeecfc, 0xb0eefc,
    0xb1f0fc, 0xb3f1fc, 0xb5f3fc, 0xb7f5fc, 0xb9f7fb, 0xbbf9fb, 0xbdfafb, 0xbffcfb,
};

struct SelState {
    unsigned prefix;   // the key's bytes fixed so far (high bytes)
    unsigned k;        // rank among the keys that match the prefix
};

struct Partial {       // one resize block
    unsigned min_key;
    unsigned has_nan;
};

struct Final {         // one image
    float vmin, vmax;
    unsigned bad;      // the map holds a NaN: every pixel takes the "bad" colour (0, 0, 0)
    unsigned pad;
};

struct VizArgs {
    const float* disp;
    float* plane;         // workspace, B * n: the resized maps
    float* resized;       // optional copy for the caller
    float* stats;         // optional (B, 2)
    unsigned char* rgb;
    unsigned* hist;       // [pass][b][rank][bin]
    SelState* state;      // [b][rank]
    Partial* part;        // [b * blocks + bx]
    Final* fin;           // [b]
    int B, h, w, H, W, n, blocks;
    float sy, sx;         // f32(h) / f32(H), f32(w) / f32(W)
    unsigned k0, k1;      // the ranks lo and lo + 1 (both n - 1 when `top`)
    float g;              // the fraction between them
    int top;              // vi >= n - 1: vmax is the maximum
};

__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float value_of(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// F.interpolate's source coordinate (align_corners=False) in fp32
__device__ __forceinline__ void lerp_coord(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i0 = i0 > in - 1 ? in - 1 : i0;       // unreachable for a finite scale; keeps the reads inside
    i1 = i0 + 1 > in - 1 ? in - 1 : i0 + 1;
    l1 = s - (float)i0;
    l0 = 1.f - l1;
}

// one count into an LDS histogram; a wave whose active lanes all hit one bin (the top byte
// of a disparity map's keys takes a handful of values) adds its population once
__device__ __forceinline__ void hist_add(unsigned* lh, unsigned bin) {
    const unsigned first = __builtin_amdgcn_readfirstlane(bin);
    const unsigned long long active = __ballot(1), same = __ballot(bin == first);
    if (same == active) {
        if ((int)__lane_id() == __ffsll((long long)active) - 1) atomicAdd(&lh[first], (unsigned)__popcll(active));
    } else {
        atomicAdd(&lh[bin], 1u);
    }
}

__device__ __forceinline__ void lds_hist_flush(const unsigned* lh, unsigned* gh) {
    for (int i = threadIdx.x; i < kRanks * kBins; i += kThreads) {
        const unsigned c = lh[i];
        if (c) atomicAdd(gh + i, c);
    }
}

// grid (blocks, B)
__global__ __launch_bounds__(kThreads) void viz_resize_kernel(VizArgs a) {
    __shared__ unsigned lh[kRanks * kBins];
    __shared__ unsigned rmin[kThreads], rnan[kThreads];
    const int t = threadIdx.x;
    for (int i = t; i < kRanks * kBins; i += kThreads) lh[i] = 0;
    __syncthreads();
    const int b = blockIdx.y;
    const float* src = a.disp + (size_t)b * a.h * a.w;
    const size_t obase = (size_t)b * a.n;
    unsigned mn = 0xFFFFFFFFu, bad = 0;
    for (int p = blockIdx.x * kThreads + t; p < a.n; p += gridDim.x * kThreads) {
        const int y = p / a.W, x = p - y * a.W;
        int y0, y1, x0, x1;
        float hy0, hy1, wx0, wx1;
        lerp_coord(y, a.sy, a.h, y0, y1, hy0, hy1);
        lerp_coord(x, a.sx, a.w, x0, x1, wx0, wx1);
        const float v00 = src[(size_t)y0 * a.w + x0], v01 = src[(size_t)y0 * a.w + x1];
        const float v10 = src[(size_t)y1 * a.w + x0], v11 = src[(size_t)y1 * a.w + x1];
        const float top = wx0 * v00 + wx1 * v01, bot = wx0 * v10 + wx1 * v11;
        const float r = hy0 * top + hy1 * bot;
        a.plane[obase + p] = r;
        if (a.resized) a.resized[obase + p] = r;
        const unsigned key = key_of(r);
        bad |= (r != r) ? 1u : 0u;
        mn = key < mn ? key : mn;
        hist_add(lh, key >> 24);
    }
    rmin[t] = mn;
    rnan[t] = bad;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (t < half) {
            rmin[t] = rmin[t + half] < rmin[t] ? rmin[t + half] : rmin[t];
            rnan[t] |= rnan[t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        Partial o;
        o.min_key = rmin[0];
        o.has_nan = rnan[0];
        a.part[(size_t)b * a.blocks + blockIdx.x] = o;
    }
    for (int i = t; i < kBins; i += kThreads) lh[kBins + i] = lh[i];   // both ranks start from the same counts
    __syncthreads();
    lds_hist_flush(lh, a.hist + (size_t)b * kRanks * kBins);
}

// grid (blocks, B): byte `3 - pass` of the keys whose higher bytes equal each rank's prefix
__global__ __launch_bounds__(kThreads) void viz_hist_kernel(VizArgs a, int pass) {
    __shared__ unsigned lh[kRanks * kBins];
    for (int i = threadIdx.x; i < kRanks * kBins; i += kThreads) lh[i] = 0;
    const int b = blockIdx.y;
    const int shift = 24 - 8 * pass;
    const unsigned want0 = a.state[b * kRanks + 0].prefix >> (shift + 8);
    const unsigned want1 = a.state[b * kRanks + 1].prefix >> (shift + 8);
    __syncthreads();
    const float* plane = a.plane + (size_t)b * a.n;
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < a.n; p += gridDim.x * kThreads) {
        const unsigned key = key_of(plane[p]);
        const unsigned hi = key >> (shift + 8), bin = (key >> shift) & 255u;
        if (hi == want0) atomicAdd(&lh[bin], 1u);
        if (hi == want1) atomicAdd(&lh[kBins + bin], 1u);
    }
    __syncthreads();
    lds_hist_flush(lh, a.hist + ((size_t)pass * a.B + b) * kRanks * kBins);
}

// grid B * kRanks, one wave each: the bin that holds rank k, and k within it
__global__ __launch_bounds__(64) void viz_select_kernel(VizArgs a, int pass) {
    const int bq = blockIdx.x, lane = threadIdx.x;
    const unsigned* h = a.hist + ((size_t)pass * a.B * kRanks + bq) * kBins + 4 * lane;
    const unsigned c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
    const unsigned mine = c0 + c1 + c2 + c3;
    unsigned incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    SelState s;
    if (pass == 0) {
        s.prefix = 0;
        s.k = (bq & 1) ? a.k1 : a.k0;
    } else {
        s = a.state[bq];
    }
    const unsigned excl = incl - mine;
    if (s.k >= excl && s.k < incl) {   // exactly one lane: the counts of a pass sum to more than k
        unsigned k = s.k - excl, d = 0;
        if (k >= c0) { k -= c0; d = 1;
            if (k >= c1) { k -= c1; d = 2;
                if (k >= c2) { k -= c2; d = 3; } } }
        s.prefix |= (unsigned)(4 * lane + d) << (24 - 8 * pass);
        s.k = k;
        a.state[bq] = s;
    }
}

// grid B, 256 threads: lane j takes block j's partial, strides 128 .. 1 fold j + stride into j
__global__ __launch_bounds__(kThreads) void viz_final_kernel(VizArgs a) {
    __shared__ unsigned rmin[kThreads], rnan[kThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    unsigned mn = 0xFFFFFFFFu, bad = 0;
    if (t < a.blocks) {
        const Partial p = a.part[(size_t)b * a.blocks + t];
        mn = p.min_key;
        bad = p.has_nan;
    }
    rmin[t] = mn;
    rnan[t] = bad;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (t < half) {
            rmin[t] = rmin[t + half] < rmin[t] ? rmin[t + half] : rmin[t];
            rnan[t] |= rnan[t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        Final f;
        f.bad = rnan[0];
        f.pad = 0;
        f.vmin = value_of(rmin[0]);
        // numpy's `linear` percentile on an fp32 array, every step fp32
        const float a0 = value_of(a.state[b * kRanks + 0].prefix), a1 = value_of(a.state[b * kRanks + 1].prefix);
        if (a.top) {
            f.vmax = a1;
        } else {
            const float d = a1 - a0;
            if (a.g >= 0.5f) {
                const float w = 1.f - a.g, prod = d * w;
                f.vmax = a1 - prod;
            } else {
                const float prod = d * a.g;
                f.vmax = a0 + prod;
            }
        }
        if (f.bad) f.vmin = f.vmax = __uint_as_float(kNan);
        a.fin[b] = f;
        if (a.stats) {
            a.stats[(size_t)b * 2] = f.vmin;
            a.stats[(size_t)b * 2 + 1] = f.vmax;
        }
    }
}

// matplotlib's Normalize and Colormap.__call__ for one value -> packed table entry
__device__ __forceinline__ unsigned colour_of(float r, const Final& f, double range, const unsigned* lut) {
    if (f.bad) return 0u;
    float tn = 0.f;
    if (f.vmin != f.vmax) {
        const float u = (float)((double)r - (double)f.vmin);
        tn = (float)((double)u / range);
    }
    const float x = tn * 256.f;
    // x == 256 -> 255, x < 0 -> under (entry 0), x >= 256 -> over (entry 255); a NaN x (from
    // an infinite range) takes entry 0 instead of indexing anywhere
    const int idx = !(x >= 0.f) ? 0 : (x >= 256.f ? 255 : (int)x);
    return lut[idx];
}

// grid (blocks, B): four consecutive pixels (12 bytes) per thread and step
__global__ __launch_bounds__(kThreads) void viz_colour_kernel(VizArgs a) {
    __shared__ unsigned lut[256];
    lut[threadIdx.x] = kMagma[threadIdx.x];   // kThreads == 256
    __syncthreads();
    const int b = blockIdx.y;
    const Final f = a.fin[b];
    const double range = (double)f.vmax - (double)f.vmin;
    const float* plane = a.plane + (size_t)b * a.n;
    unsigned char* out = a.rgb + (size_t)b * a.n * 3;
    const int quads = (a.n + 3) / 4;
    for (int q = blockIdx.x * kThreads + threadIdx.x; q < quads; q += gridDim.x * kThreads) {
        const int p0 = q * 4;
        unsigned char* dst = out + (size_t)p0 * 3;
        if (p0 + 4 <= a.n && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
            const unsigned c0 = colour_of(plane[p0], f, range, lut), c1 = colour_of(plane[p0 + 1], f, range, lut);
            const unsigned c2 = colour_of(plane[p0 + 2], f, range, lut), c3 = colour_of(plane[p0 + 3], f, range, lut);
            unsigned* d32 = reinterpret_cast<unsigned*>(dst);
            d32[0] = c0 | (c1 << 24);
            d32[1] = (c1 >> 8) | (c2 << 16);
            d32[2] = (c2 >> 16) | (c3 << 8);
        } else {   // an image whose bytes start off a dword boundary (odd H * W), or the tail
            const int end = p0 + 4 < a.n ? p0 + 4 : a.n;
            for (int p = p0; p < end; ++p) {
                const unsigned c = colour_of(plane[p], f, range, lut);
                out[(size_t)p * 3] = (unsigned char)(c & 255u);
                out[(size_t)p * 3 + 1] = (unsigned char)((c >> 8) & 255u);
                out[(size_t)p * 3 + 2] = (unsigned char)((c >> 16) & 255u);
            }
        }
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Layout {
    size_t plane, hist, state, part, fin, total;
    int n, blocks;
};

const char* check_desc(const md2_viz_desc* d) {
    if (!d) return "disp_colorize: NULL desc";
    if (d->batch < 1 || d->in_height < 1 || d->in_width < 1 || d->out_height < 1 || d->out_width < 1)
        return "disp_colorize: batch, in_height, in_width, out_height, out_width must be positive";
    if (d->batch > kMaxBatch) return "disp_colorize: batch too large (at most 65535 images per call)";
    if ((long long)d->out_height * d->out_width > kMaxPixels)
        return "disp_colorize: out_height * out_width above 2^24 (the percentile's fp32 rank must be exact)";
    if ((long long)d->in_height * d->in_width >= (1ll << 31)) return "disp_colorize: in_height * in_width at or above 2^31";
    if (d->percentile < 0 || d->percentile > 100) return "disp_colorize: percentile must be 0..100";
    if (d->flags) return "disp_colorize: unknown flags (none are defined)";
    return nullptr;
}

Layout layout(const md2_viz_desc* d) {
    Layout l;
    l.n = d->out_height * d->out_width;
    const int want = (l.n + kThreads * kPixelsPerThread - 1) / (kThreads * kPixelsPerThread);
    l.blocks = want < 1 ? 1 : (want > kMaxBlocksPerImage ? kMaxBlocksPerImage : want);
    size_t off = 0;
    l.plane = off; off += align256(sizeof(float) * (size_t)d->batch * l.n);
    l.hist = off;  off += align256(sizeof(unsigned) * (size_t)kPasses * d->batch * kRanks * kBins);
    l.state = off; off += align256(sizeof(SelState) * (size_t)d->batch * kRanks);
    l.part = off;  off += align256(sizeof(Partial) * (size_t)d->batch * l.blocks);
    l.fin = off;   off += align256(sizeof(Final) * (size_t)d->batch);
    l.total = off;
    return l;
}

}  // namespace

extern "C" {

size_t md2_disp_colorize_workspace_bytes(const md2_viz_desc* d) {
    if (const char* msg = check_desc(d)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return layout(d).total;
}

int md2_disp_colorize(const md2_viz_desc* d, const float* disp, uint8_t* rgb, float* resized, float* stats,
                      void* workspace, void* stream) {
    if (const char* msg = check_desc(d)) return md2_report_error(MD2_ERR_ARG, msg);
    if (!disp || !rgb || !workspace) return md2_report_error(MD2_ERR_ARG, "disp_colorize: NULL operand");
    if (reinterpret_cast<uintptr_t>(workspace) % 256)
        return md2_report_error(MD2_ERR_ARG, "disp_colorize: workspace must be 256-byte aligned");
    const Layout l = layout(d);
    char* ws = static_cast<char*>(workspace);
    VizArgs a = {};
    a.disp = disp;
    a.plane = reinterpret_cast<float*>(ws + l.plane);
    a.resized = resized;
    a.stats = stats;
    a.rgb = rgb;
    a.hist = reinterpret_cast<unsigned*>(ws + l.hist);
    a.state = reinterpret_cast<SelState*>(ws + l.state);
    a.part = reinterpret_cast<Partial*>(ws + l.part);
    a.fin = reinterpret_cast<Final*>(ws + l.fin);
    a.B = d->batch; a.h = d->in_height; a.w = d->in_width; a.H = d->out_height; a.W = d->out_width;
    a.n = l.n; a.blocks = l.blocks;
    a.sy = (float)d->in_height / (float)d->out_height;
    a.sx = (float)d->in_width / (float)d->out_width;
    // numpy's `linear` method: the virtual index (n - 1) * q in fp32, its floor and fraction
    const float last = (float)(l.n - 1);
    const float q = (float)d->percentile / 100.f;
    const float vi = last * q;
    if (vi >= last) {
        a.top = 1;
        a.k0 = a.k1 = (unsigned)(l.n - 1);
        a.g = 0.f;
    } else {
        const float lo = floorf(vi);
        a.top = 0;
        a.k0 = (unsigned)lo;
        a.k1 = a.k0 + 1;
        a.g = vi - lo;
    }

    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(l.blocks, d->batch), block(kThreads);
    hipError_t e = hipMemsetAsync(a.hist, 0, sizeof(unsigned) * (size_t)kPasses * d->batch * kRanks * kBins, st);
    if (e != hipSuccess) return md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
    hipLaunchKernelGGL(viz_resize_kernel, grid, block, 0, st, a);
    for (int pass = 0; pass < kPasses; ++pass) {
        if (pass > 0) hipLaunchKernelGGL(viz_hist_kernel, grid, block, 0, st, a, pass);
        hipLaunchKernelGGL(viz_select_kernel, dim3(d->batch * kRanks), dim3(64), 0, st, a, pass);
    }
    hipLaunchKernelGGL(viz_final_kernel, dim3(d->batch), block, 0, st, a);
    hipLaunchKernelGGL(viz_colour_kernel, grid, block, 0, st, a);
    e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
