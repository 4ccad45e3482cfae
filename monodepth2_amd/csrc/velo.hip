// velo.hip — KITTI velodyne scans -> sparse ground-truth depth maps on gfx950.
//
// Reference: kitti_utils.generate_depth_map (kitti_utils.py:46-98) projects the points of
// one scan into a camera with numpy, writes them into the map with a fancy assignment
// (the last point of a pixel wins) and then resolves duplicates in a Python loop: points
// are grouped by sub2ind = v * (W - 1) + u - 1, and the pixel of a group's first point
// receives the group's minimum depth.  That key is not the pixel index: (v, W-1) and
// (v+1, 0) share it, so of such a pair of pixels the one hit first (in point order) gets
// the minimum over both, and the other keeps its last-written value.  export_gt_depth.py
// runs this once per test frame.  Here (md2_velo_project, include/md2hot.h) a batch of
// scans is a fixed chain of three launches:
//
//   memset    the per-pixel records
//   scatter   one thread per point, the frame on grid.y: fp64 projection, rounding,
//             bounds; three integer atomics into the pixel's record
//   resolve   one thread per pixel: the rules above from its own record and the record
//             of its wrap partner (columns 0 and W-1), negative -> 0, the fp32 map
//
// A record holds, for the valid points of a pixel, three maxima (so that zero means
// "none" and one memset initialises them):
//   last    (index + 1) << 32 | depth bits      the last point and its value
//   nmin    ~key(depth), key order-preserving   the smallest depth
//   nfirst  ~index                              the first point
// The point index within the frame is the point order (the reference's filters keep the
// relative order), so nothing is compacted.  Integer maxima commute: the result does not
// depend on the order the atomics arrive in, and is bitwise repeatable.  The reference's
// duplicate count is not needed: a pixel whose group holds one point has minimum = last.
//
// Arithmetic: the projection is fp64 with the products and sums in the written order and
// no contraction, as numpy's dot of a 3x4 by a 4-vector evaluates it without BLAS; u and
// v are compared with the bounds in fp64 before any conversion, so NaN, infinite and
// q2 == 0 points fall out through the comparisons alone.  The map is fp32 (what
// export_gt_depth.py stores): rounding is monotone, so rounding each depth first and
// taking the minimum of the rounded values is the rounded minimum.

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBatch = 65535;          // frames are grid.y
constexpr int kMaxScatterBlocks = 512;    // per frame; longer frames loop

struct alignas(16) Record {
    unsigned long long last;
    unsigned nmin;
    unsigned nfirst;
};

struct VeloArgs {
    const float* points;
    const long long* offsets;
    const double* P;
    Record* rec;
    float* depth;
    long long total;
    int B, H, W, npix;
    unsigned flags;
};

// fp32 -> uint32, monotone: a < b <=> key(a) < key(b) (-0.0 below +0.0; no NaN gets here)
__device__ __forceinline__ unsigned order_key(float f) {
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float order_value(unsigned k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

__device__ __forceinline__ double dot4(const double* p, double x, double y, double z) {
#pragma clang fp contract(off)
    return ((p[0] * x + p[1] * y) + p[2] * z) + p[3];
}

// grid (blocks, B)
__global__ __launch_bounds__(kThreads) void velo_scatter_kernel(VeloArgs a) {
    const int b = blockIdx.y;
    // the contract is 0 = offsets[0] <= ... <= offsets[B] = total; the clamp keeps a
    // broken table from reading outside `points` (the maps are then meaningless)
    long long begin = a.offsets[b], end = a.offsets[b + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > a.total ? a.total : end;
    double p[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = a.P[(size_t)b * 12 + i];
    Record* rec = a.rec + (size_t)b * a.npix;
    const bool vel = a.flags & MD2_VELO_VEL_DEPTH;
    const double fw = (double)a.W, fh = (double)a.H;
    for (long long i = begin + (long long)blockIdx.x * kThreads + threadIdx.x; i < end;
         i += (long long)gridDim.x * kThreads) {
        const float* pt = a.points + (size_t)i * 4;
        const float xf = pt[0], yf = pt[1], zf = pt[2];
        if (!(xf >= 0.f)) continue;                      // kitti_utils.py:67 (NaN fails it too)
        const double x = xf, y = yf, z = zf;
        const double q0 = dot4(p, x, y, z), q1 = dot4(p + 4, x, y, z), q2 = dot4(p + 8, x, y, z);
        const double u = rint(q0 / q2) - 1.0, v = rint(q1 / q2) - 1.0;   // np.round: half to even
        if (!(u >= 0.0 && v >= 0.0 && u < fw && v < fh)) continue;
        float d;
        if (vel) {
            d = xf;
        } else {
            // every negative depth ends as 0 whatever its size (kitti_utils.py:96, applied to
            // the fp64 map); fp32 rounding could turn a tiny one into -0.0, which is not < 0
            d = q2 < 0.0 ? -1.f : (float)q2;
        }
        const unsigned idx = (unsigned)(i - begin);
        Record* r = rec + ((int)v * a.W + (int)u);
        atomicMax(&r->last, ((unsigned long long)(idx + 1u) << 32) | __float_as_uint(d));
        atomicMax(&r->nmin, ~order_key(d));
        atomicMax(&r->nfirst, ~idx);
    }
}

// one thread per pixel of the batch
__global__ __launch_bounds__(kThreads) void velo_resolve_kernel(VeloArgs a) {
    const int total = a.B * a.npix;
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= total) return;
    const int pix = g % a.npix;
    const int v = pix / a.W, u = pix - v * a.W;
    const Record own = a.rec[g];
    float out = 0.f;
    if (own.last != 0ull) {
        // the other pixel with this pixel's sub2ind key, if any (W >= 2: at most one)
        int partner = -1;
        if (u == 0 && v > 0) partner = g - 1;                     // (v-1, W-1)
        else if (u == a.W - 1 && v < a.H - 1) partner = g + 1;    // (v+1, 0)
        unsigned nmin = own.nmin;
        bool first = true;
        if (partner >= 0) {
            const Record o = a.rec[partner];
            if (o.last != 0ull) {
                first = own.nfirst > o.nfirst;                    // ~index: larger = earlier
                nmin = nmin > o.nmin ? nmin : o.nmin;
            }
        }
        out = first ? order_value(~nmin) : __uint_as_float((unsigned)own.last);
        if (out < 0.f) out = 0.f;
    }
    a.depth[g] = out;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

const char* check_desc(const md2_velo_desc* d) {
    if (!d) return "velo_project: NULL desc";
    if (d->batch < 1 || d->height < 1 || d->width < 1 || d->total_points < 1)
        return "velo_project: batch, height, width, total_points must be positive";
    if (d->width < 2) return "velo_project: width must be at least 2 (the duplicate key degenerates below)";
    if (d->batch > kMaxBatch) return "velo_project: batch too large (at most 65535 frames per call)";
    // headroom of one block below 2^31, so the resolve kernel's int index cannot overflow
    if ((long long)d->batch * d->height * d->width >= (1ll << 31) - kThreads)
        return "velo_project: batch too large (2^31 pixels)";
    if (d->total_points >= (1ll << 31)) return "velo_project: too many points (2^31)";
    if (d->flags & ~(uint32_t)MD2_VELO_VEL_DEPTH) return "velo_project: unknown flags";
    return nullptr;
}

}  // namespace

extern "C" {

size_t md2_velo_project_workspace_bytes(const md2_velo_desc* d) {
    if (const char* msg = check_desc(d)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return align256(sizeof(Record) * (size_t)d->batch * d->height * d->width);
}

int md2_velo_project(const md2_velo_desc* d, const float* points, const int64_t* offsets, const double* P,
                     float* depth, void* workspace, void* stream) {
    if (const char* msg = check_desc(d)) return md2_report_error(MD2_ERR_ARG, msg);
    if (!points || !offsets || !P || !depth || !workspace)
        return md2_report_error(MD2_ERR_ARG, "velo_project: NULL operand");
    if (reinterpret_cast<uintptr_t>(workspace) % alignof(Record))
        return md2_report_error(MD2_ERR_ARG, "velo_project: workspace must be 16-byte aligned");
    VeloArgs a = {};
    a.points = points;
    a.offsets = reinterpret_cast<const long long*>(offsets);
    a.P = P;
    a.rec = static_cast<Record*>(workspace);
    a.depth = depth;
    a.total = d->total_points;
    a.B = d->batch; a.H = d->height; a.W = d->width; a.npix = d->height * d->width;
    a.flags = d->flags;

    const hipStream_t st = (hipStream_t)stream;
    const size_t pixels = (size_t)d->batch * a.npix;
    const hipError_t m = hipMemsetAsync(a.rec, 0, sizeof(Record) * pixels, st);
    if (m != hipSuccess) return md2_report_error(MD2_ERR_HIP, hipGetErrorString(m));
    // twice the mean frame's worth of threads per frame; a longer frame strides
    const long long mean = (d->total_points + d->batch - 1) / d->batch;
    long long blocks = (2 * mean + kThreads - 1) / kThreads;
    blocks = blocks < 1 ? 1 : (blocks > kMaxScatterBlocks ? kMaxScatterBlocks : blocks);
    hipLaunchKernelGGL(velo_scatter_kernel, dim3((unsigned)blocks, d->batch), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(velo_resolve_kernel, dim3((unsigned)((pixels + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
