// points.hip — predicted depth as a point cloud on gfx950: a batch of maps at the original
// image size -> the packed 15-byte vertex records of a binary PLY file, so that the device
// buffer is the file body (md2_depth_points, include/md2hot.h).
//
// Reference: disp_to_depth (layers.py:16-25) and BackprojectDepth (layers.py:139-168), fp32
// per pixel; velo.hip is the opposite direction (points -> depth maps).  New here: pixels
// off the stride grid, out of [near, far] or not finite are dropped, the survivors are
// compacted in (image, row, column) order over the whole batch, and each is packed as
// x, y, z (float32) + red, green, blue.  Three launches on the caller's stream, a block on
// kCand candidates of one image (grid.x), the image on grid.y:
//
//   count   every candidate evaluated; per block the number kept -> workspace
//   scan    one block: exclusive scan of the block counts in block order (image-major), in
//           place; the running total at each image's end -> offsets
//   emit    every candidate evaluated again (the same inlined expressions: the same bits);
//           rank inside the block from 64-bit ballots + mbcnt in (pass, wave, lane) order;
//           records assembled in LDS, then the block's byte range 15 * slot .. written as
//           whole dwords where a dword lies inside it and as bytes at its head and tail
//
// A record's slot comes from the scan, never from an atomic counter: the order is part of
// the contract.  No atomics at all, no float reduction: bitwise repeatable.
//
// Arithmetic.  Every product and sum is a separately rounded fp32 operation in the written
// order (no contraction) and the division is the correctly rounded one of the default
// flags, so tests/points_case.py restates the operator in numpy bit for bit.
//
// Bounds.  slot + rank < the candidates before the block + the candidates in it <= the
// batch's candidates <= capacity (checked on the host), whatever the predicate gives: no
// record can land past `capacity`.  The colour dwords are read only where the whole dword
// lies inside the rgb operand (else three byte loads: the operand's last pixel at most).

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPasses = 4;                      // candidates per thread
constexpr int kCand = kThreads * kPasses;       // candidates per block
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 8;                   // consecutive block counts per scan thread
constexpr int kMaxBatch = 65535;                // images are grid.y
constexpr unsigned kRecord = 15;                // bytes: 3 x float32 + 3 x uint8
constexpr unsigned kFlags = MD2_POINTS_DEPTH_INPUT | MD2_POINTS_WORLD;

struct PointsArgs {
    const float* map;
    const unsigned char* rgb;
    const float* inv_K;
    const float* T;
    unsigned char* vertices;
    unsigned* offsets;
    unsigned* slots;            // workspace: block counts, then their exclusive scan
    int B, H, W, stride;
    int Hs, Ws;                 // the stride grid: ceil(H / stride), ceil(W / stride)
    unsigned nc;                // Hs * Ws candidates per image
    unsigned bpi;               // blocks per image
    unsigned long long rgb_bytes;   // 3 * B * H * W
    int rgb_words;              // the rgb operand is dword aligned: colours come as dwords
    float disp_a, disp_b, depth_scale, near, far;
    int depth_input, world;
};

struct Camera {
    float k[3][3];
    float t[3][4];
};

__device__ __forceinline__ Camera load_camera(const PointsArgs& a, int b) {
    Camera c;
    const float* k = a.inv_K + (size_t)b * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.k[i][j] = k[i * 4 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) c.t[i][j] = a.world ? a.T[(size_t)b * 16 + i * 4 + j] : 0.f;
    return c;
}

__device__ __forceinline__ bool finite_f32(float v) {
    return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u;
}

// the contract's steps 1-6 for map value d at pixel (x, y); false: the pixel is dropped
__device__ __forceinline__ bool point_of(const PointsArgs& a, const Camera& c, float d, int x, int y, float out[3]) {
    float depth = d;
    if (!a.depth_input) {
        const float sd = a.disp_b + a.disp_a * d;
        depth = 1.0f / sd;
    }
    const float z = a.depth_scale * depth;
    const float fx = (float)x, fy = (float)y;
    float p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float r = (c.k[i][0] * fx + c.k[i][1] * fy) + c.k[i][2];
        p[i] = z * r;
    }
    if (a.world) {
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = ((c.t[i][0] * p[0] + c.t[i][1] * p[1]) + c.t[i][2] * p[2]) + c.t[i][3];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) out[i] = p[i];
    }
    return z >= a.near && z <= a.far && finite_f32(out[0]) && finite_f32(out[1]) && finite_f32(out[2]);
}

// candidate c of an image -> its pixel; the map value is read only for a real candidate
__device__ __forceinline__ bool candidate(const PointsArgs& a, const Camera& cam, size_t image, unsigned c,
                                          float out[3], size_t& pixel) {
    if (c >= a.nc) return false;
    const unsigned row = c / (unsigned)a.Ws;
    const int y = (int)row * a.stride, x = (int)(c - row * (unsigned)a.Ws) * a.stride;
    pixel = image + (size_t)y * a.W + x;
    return point_of(a, cam, a.map[pixel], x, y, out);
}

__device__ __forceinline__ unsigned lane_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// grid (bpi, B)
__global__ __launch_bounds__(kThreads) void points_count_kernel(PointsArgs a) {
    __shared__ unsigned wc[kPasses * kWaves];
    const int b = blockIdx.y, t = threadIdx.x;
    const Camera cam = load_camera(a, b);
    const size_t image = (size_t)b * a.H * a.W;
    const unsigned long long c0 = (unsigned long long)blockIdx.x * kCand;
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
        const unsigned long long c = c0 + (unsigned)(k * kThreads + t);
        float p[3];
        size_t pixel;
        const bool keep = c < a.nc && candidate(a, cam, image, (unsigned)c, p, pixel);
        const unsigned long long mask = __ballot(keep);
        if ((t & 63) == 0) wc[k * kWaves + (t >> 6)] = (unsigned)__popcll(mask);
    }
    __syncthreads();
    if (t == 0) {
        unsigned n = 0;
#pragma unroll
        for (int i = 0; i < kPasses * kWaves; ++i) n += wc[i];
        a.slots[(size_t)b * a.bpi + blockIdx.x] = n;
    }
}

// one block: slots[i] <- sum of slots[0 .. i-1], chunk after chunk with a carry (a thread
// sums kScanItems consecutive counts, the waves scan the thread sums); then offsets
__global__ __launch_bounds__(kScanThreads) void points_scan_kernel(PointsArgs a) {
    __shared__ unsigned wsum[kScanThreads / 64];
    __shared__ unsigned carry_s;
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long total = (unsigned long long)a.B * a.bpi;   // below 2^22 + 2^16
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (unsigned long long base = 0; base < total; base += kScanThreads * kScanItems) {
        const unsigned long long i0 = base + (unsigned long long)t * kScanItems;
        unsigned v[kScanItems], mine = 0;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            v[k] = i0 + k < total ? a.slots[i0 + k] : 0u;
            mine += v[k];
        }
        unsigned incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(incl, d, 64);
            if (lane >= (unsigned)d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = carry_s;
        for (unsigned w = 0; w < wave; ++w) before += wsum[w];
        unsigned run = before + incl - mine;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            if (i0 + k < total) a.slots[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (t == kScanThreads - 1) carry_s = run;
        __syncthreads();
    }
    // image b's records end where image b + 1's first block starts (this block's own stores,
    // ordered by the barrier above)
    for (unsigned b = t; b < (unsigned)a.B; b += kScanThreads)
        a.offsets[b + 1] = b + 1 < (unsigned)a.B ? a.slots[(size_t)(b + 1) * a.bpi] : carry_s;
    if (t == 0) a.offsets[0] = 0;
}

// a pixel's three bytes, packed red | green << 8 | blue << 16
__device__ __forceinline__ unsigned colour_of(const PointsArgs& a, size_t pixel) {
    const unsigned long long at = (unsigned long long)pixel * 3;
    const unsigned long long w0 = at >> 2, w1 = (at + 2) >> 2;
    if (a.rgb_words && (w1 + 1) * 4 <= a.rgb_bytes) {   // two aligned dwords (often one) hold them
        const unsigned* words = reinterpret_cast<const unsigned*>(a.rgb);
        const unsigned lo = words[w0], hi = words[w1];
        const unsigned sh = (unsigned)(at & 3) * 8;
        return (unsigned)((((unsigned long long)hi << 32 | lo) >> sh) & 0xFFFFFFu);
    }
    return (unsigned)a.rgb[at] | (unsigned)a.rgb[at + 1] << 8 | (unsigned)a.rgb[at + 2] << 16;
}

// grid (bpi, B)
__global__ __launch_bounds__(kThreads) void points_emit_kernel(PointsArgs a) {
    __shared__ uint4 rec[kCand];                 // x, y, z bits and the packed colour, by rank
    __shared__ unsigned wc[kPasses * kWaves];
    const int b = blockIdx.y, t = threadIdx.x;
    const Camera cam = load_camera(a, b);
    const size_t image = (size_t)b * a.H * a.W;
    const unsigned long long c0 = (unsigned long long)blockIdx.x * kCand;
    float p[kPasses][3];
    size_t pixel[kPasses];
    bool keep[kPasses];
    unsigned rank[kPasses];
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
        const unsigned long long c = c0 + (unsigned)(k * kThreads + t);
        pixel[k] = 0;
        keep[k] = c < a.nc && candidate(a, cam, image, (unsigned)c, p[k], pixel[k]);
        const unsigned long long mask = __ballot(keep[k]);
        rank[k] = lane_rank(mask);
        if ((t & 63) == 0) wc[k * kWaves + (t >> 6)] = (unsigned)__popcll(mask);
    }
    __syncthreads();
    unsigned cnt = 0;
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
        unsigned before = 0;
#pragma unroll
        for (int i = 0; i < kPasses * kWaves; ++i) {
            const unsigned n = wc[i];
            if (i < k * kWaves + (t >> 6)) before += n;
            if (k == 0) cnt += n;
        }
        if (keep[k]) {
            const unsigned colour = colour_of(a, pixel[k]);
            rec[before + rank[k]] = make_uint4(__float_as_uint(p[k][0]), __float_as_uint(p[k][1]),
                                               __float_as_uint(p[k][2]), colour);
        }
    }
    __syncthreads();
    if (cnt == 0) return;

    // the block's bytes [0, 15 * cnt) go to dst; the dwords are aligned as the address is
    const unsigned* words = reinterpret_cast<const unsigned*>(rec);
    unsigned char* dst = a.vertices + (unsigned long long)kRecord * a.slots[(size_t)b * a.bpi + blockIdx.x];
    const int nbytes = (int)(kRecord * cnt);
    const int shift = (int)(reinterpret_cast<uintptr_t>(dst) & 3);
    const int ndw = (shift + nbytes + 3) >> 2;
    for (int j = t; j < ndw; j += kThreads) {
        const int rel0 = 4 * j - shift;
        if (rel0 >= 0 && rel0 + 4 <= nbytes) {
            // a whole dword: bytes f .. f + 3 of the 19-byte run "record r, then the next
            // record's x" (the next record exists whenever f + 3 reaches past byte 14)
            const unsigned r = (unsigned)rel0 / kRecord, f = (unsigned)rel0 - r * kRecord;
            const uint4 cur = rec[r];
            const unsigned nx = rec[r + 1 < (unsigned)kCand ? r + 1 : r].x;
            const unsigned s3 = (cur.w & 0xFFFFFFu) | (nx << 24), s4 = nx >> 8;
            const unsigned q = f >> 2;
            const unsigned lo = q == 0 ? cur.x : (q == 1 ? cur.y : (q == 2 ? cur.z : s3));
            const unsigned hi = q == 0 ? cur.y : (q == 1 ? cur.z : (q == 2 ? s3 : s4));
            *reinterpret_cast<unsigned*>(dst + rel0) = (unsigned)((((unsigned long long)hi << 32) | lo) >> ((f & 3) * 8));
        } else {                                  // the head and the tail: at most three bytes each
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rel = rel0 + i;
                if (rel >= 0 && rel < nbytes) {
                    const unsigned r = (unsigned)rel / kRecord, f = (unsigned)rel - r * kRecord;
                    dst[rel] = (unsigned char)(words[4 * r + (f >> 2)] >> ((f & 3) * 8));
                }
            }
        }
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

bool good(float v) { return isfinite(v); }

struct Layout {
    long long candidates;   // of the whole batch: the capacity a call needs
    int Hs, Ws;
    unsigned nc, bpi;
    size_t total;
};

const char* check_desc(const md2_points_desc* d, Layout* l) {
    if (!d) return "depth_points: NULL desc";
    if (d->batch < 1 || d->height < 1 || d->width < 1 || d->stride < 1)
        return "depth_points: batch, height, width, stride must be positive";
    if (d->batch > kMaxBatch) return "depth_points: batch too large (at most 65535 images per call)";
    if (d->flags & ~kFlags) return "depth_points: unknown flags";
    if (d->reserved[0] || d->reserved[1]) return "depth_points: reserved words must be 0";
    if (!good(d->depth_scale) || !(d->depth_scale > 0.f)) return "depth_points: depth_scale must be positive and finite";
    if (!good(d->near) || !good(d->far) || !(d->near > 0.f) || d->near > d->far)
        return "depth_points: near and far must be finite with 0 < near <= far";
    const long long Hs = ((long long)d->height + d->stride - 1) / d->stride;
    const long long Ws = ((long long)d->width + d->stride - 1) / d->stride;
    const long long nc = Hs * Ws;                                   // below 2^62
    if (nc >= (1ll << 31) || nc * d->batch >= (1ll << 31))
        return "depth_points: batch * ceil(height / stride) * ceil(width / stride) at or above 2^31";
    l->candidates = nc * d->batch;
    l->Hs = (int)Hs;
    l->Ws = (int)Ws;
    l->nc = (unsigned)nc;
    l->bpi = (unsigned)((nc + kCand - 1) / kCand);
    l->total = align256(sizeof(unsigned) * (size_t)d->batch * l->bpi);
    return nullptr;
}

}  // namespace

extern "C" {

size_t md2_depth_points_workspace_bytes(const md2_points_desc* d) {
    Layout l;
    if (const char* msg = check_desc(d, &l)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return l.total;
}

int md2_depth_points(const md2_points_desc* d, const float* map, const uint8_t* rgb, const float* inv_K,
                     const float* T, uint8_t* vertices, size_t capacity, uint32_t* offsets, void* workspace,
                     void* stream) {
    Layout l;
    if (const char* msg = check_desc(d, &l)) return md2_report_error(MD2_ERR_ARG, msg);
    if (!map || !rgb || !inv_K || !vertices || !offsets || !workspace)
        return md2_report_error(MD2_ERR_ARG, "depth_points: NULL operand");
    const bool world = (d->flags & MD2_POINTS_WORLD) != 0;
    if (world && !T) return md2_report_error(MD2_ERR_ARG, "depth_points: MD2_POINTS_WORLD needs T");
    if (!world && T) return md2_report_error(MD2_ERR_ARG, "depth_points: T must be NULL without MD2_POINTS_WORLD");
    if (capacity < (size_t)l.candidates)
        return md2_report_error(MD2_ERR_ARG, "depth_points: capacity below batch * ceil(height / stride) * "
                                             "ceil(width / stride) records");
    if (reinterpret_cast<uintptr_t>(workspace) % 256)
        return md2_report_error(MD2_ERR_ARG, "depth_points: workspace must be 256-byte aligned");

    PointsArgs a = {};
    a.map = map;
    a.rgb = rgb;
    a.inv_K = inv_K;
    a.T = T;
    a.vertices = vertices;
    a.offsets = offsets;
    a.slots = static_cast<unsigned*>(workspace);
    a.B = d->batch; a.H = d->height; a.W = d->width; a.stride = d->stride;
    a.Hs = l.Hs; a.Ws = l.Ws; a.nc = l.nc; a.bpi = l.bpi;
    a.rgb_bytes = 3ull * (unsigned long long)d->batch * (unsigned long long)d->height * (unsigned long long)d->width;
    a.rgb_words = reinterpret_cast<uintptr_t>(rgb) % 4 == 0;
    a.disp_a = d->disp_a; a.disp_b = d->disp_b; a.depth_scale = d->depth_scale;
    a.near = d->near; a.far = d->far;
    a.depth_input = (d->flags & MD2_POINTS_DEPTH_INPUT) != 0;
    a.world = world;

    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(l.bpi, d->batch), block(kThreads);
    hipLaunchKernelGGL(points_count_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, a);
    hipLaunchKernelGGL(points_emit_kernel, grid, block, 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
