// eval.hip — KITTI depth evaluation on gfx950: the seven Eigen metrics of a batch of
// predicted disparities against sparse ground truth, without leaving the device.
//
// Reference: evaluate_depth.py:181-214 runs, per image on the CPU, cv2.resize of the
// disparity to the ground-truth map, a boolean mask, two np.median calls, a clamp and
// compute_errors (27-45); Trainer.compute_depth_losses (trainer.py:498-526) is the same
// on the GPU with boolean indexing and torch.median — data-dependent shapes and host
// syncs.  Here (md2_depth_eval, include/md2hot.h) the work is a fixed chain of launches:
//
//   memset        the radix histograms
//   predict       one thread per ground-truth pixel: post-process + disp_to_depth +
//                 bilinear resize + mask; pred -> workspace plane (0xFFFFFFFF = invalid);
//                 histogram of the top byte of the valid pred / gt bit patterns
//   select x4     per (population, array, rank): the bin holding the k-th key, k reduced
//   hist   x3     histogram of the next byte of the keys that match the prefix so far
//   reduce        pred * ratio, clamp, the seven sums: per thread, then a fixed LDS tree
//   finalise      block partials summed in block order in fp64, means and roots
//
// Arithmetic.  disp_to_depth is torch's fp32 multiply and add (the reference's evaluation
// starts from that fp32 array); everything after it — post-processing, resize, inversion —
// runs in fp64 per valid pixel and is rounded once to the fp32 prediction the medians
// select from.  The error terms and their sums are fp64 as well (fp32 block trees were
// the first plan: their rounding alone, ~1e-7 relative, is the size of the whole fp32
// numpy formulation's error, which is the yardstick of tests/test_eval_gpu.py).  The op is
// bandwidth-bound at a few hundred fp64 operations per valid pixel.
//
// Positive floats order as their bit patterns, so the k-th smallest value is the k-th
// smallest uint32 key: four 8-bit passes give the exact order statistic.  Four selection
// problems per population (pred / gt x rank (n-1)/2 / rank n/2) run side by side; the
// median convention picks from them at the end.  Histograms and counts are integer
// atomics (they commute); no float atomic anywhere, so results are bitwise repeatable.
// Without MD2_EVAL_MEDIAN_SCALE the chain is predict, reduce, finalise.
//
// md2_depth_export16 (further down) is the `benchmark` split's 16-bit depth export on the
// same prediction: one launch, no workspace.

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

namespace {

constexpr int kThreads = 256;
constexpr int kBins = 256;
constexpr int kProblems = 4;             // (pred, gt) x (rank (n-1)/2, rank n/2): index arr * 2 + which
constexpr int kPasses = 4;
constexpr unsigned kInvalid = 0xFFFFFFFFu;
constexpr unsigned kEmpty = 0xFFFFFFFFu; // SelState.k of a population without valid pixels
constexpr int kMaxBlocksPerImage = 64;   // reduce / histogram blocks per image
constexpr int kPixelsPerThread = 8;
constexpr int kMaxBatch = 65535;         // images are grid.y

struct SelState {
    unsigned prefix;   // the key's bytes fixed so far (high bytes)
    unsigned k;        // rank among the keys that match the prefix
    unsigned n;        // valid pixels of the population
    unsigned pad;
};

struct Partial {       // one reduce block
    double sum[4];     // |gt - pred| / gt, (gt - pred)^2 / gt, (gt - pred)^2, log(gt / pred)^2
    unsigned cnt[4];   // a1, a2, a3, valid pixels
};

struct EvalArgs {
    const float* disp;
    const float* dispf;
    const float* gt;
    unsigned* pred;       // workspace plane, B * npix
    unsigned* hist;       // [pass][pop][problem][bin]
    SelState* state;      // [pop][problem]
    Partial* part;        // [b * blocks + bx]
    float* out;
    int B, h, w, GH, GW, npix, P, blocks;
    int y0, y1, x0, x1;
    unsigned flags;
    float lo, range;      // scaled = lo + range * disp
    float emin, emax;
    double sf;
    double sy, sx;        // h / GH, w / GW
};

__device__ __forceinline__ double pp_mask(int x, int w) {
    const double l = w > 1 ? (double)x / (double)(w - 1) : 0.0;
    return 1.0 - fmin(fmax(20.0 * (l - 0.05), 0.0), 1.0);
}

// layers.py:16-25 as torch evaluates it: an fp32 product rounded, then an fp32 sum — the
// pragma keeps the compiler from fusing the two (__fmul_rn / __fadd_rn alone are fused
// under hipcc's default -ffp-contract=fast-honor-pragmas)
__device__ __forceinline__ float disp_to_scaled(float lo, float range, float disp) {
#pragma clang fp contract(off)
    const float prod = range * disp;
    return lo + prod;
}

// the scaled disparity of network pixel (y, x) of image b, post-processed if asked
// (evaluate_depth.py:48-56; the flipped pass is read mirrored)
template <bool PP>
__device__ __forceinline__ double scaled_disp(const EvalArgs& a, size_t base, int y, int x) {
    const double d = disp_to_scaled(a.lo, a.range, a.disp[base + (size_t)y * a.w + x]);
    if (!PP) return d;
    const double df = disp_to_scaled(a.lo, a.range, a.dispf[base + (size_t)y * a.w + (a.w - 1 - x)]);
    const double lm = pp_mask(x, a.w), rm = pp_mask(a.w - 1 - x, a.w);
    return rm * d + lm * df + (1.0 - lm - rm) * (0.5 * (d + df));
}

__device__ __forceinline__ void lerp_coord(int dst, double scale, int in, int& i0, int& i1, double& f) {
    double s = scale * ((double)dst + 0.5) - 0.5;
    s = s < 0.0 ? 0.0 : s;
    i0 = (int)s;
    i0 = i0 > in - 1 ? in - 1 : i0;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    f = s - (double)i0;
}

__device__ __forceinline__ void lds_hist_flush(const unsigned* lh, unsigned* gh) {
    for (int i = threadIdx.x; i < kProblems * kBins; i += kThreads) {
        const unsigned c = lh[i];
        if (c) atomicAdd(gh + i, c);
    }
}

// grid (blocks, B).  Pass-0 histograms: both ranks of an array see the same keys.
template <bool PP, bool DEPTH>
__global__ __launch_bounds__(kThreads) void eval_predict_kernel(EvalArgs a) {
    __shared__ unsigned lh[kProblems * kBins];
    const bool median = a.flags & MD2_EVAL_MEDIAN_SCALE;
    if (median) {
        for (int i = threadIdx.x; i < kProblems * kBins; i += kThreads) lh[i] = 0;
        __syncthreads();
    }
    const int b = blockIdx.y;
    const size_t dbase = (size_t)b * a.h * a.w, gbase = (size_t)b * a.npix;
    const bool range = a.flags & MD2_EVAL_GT_RANGE;
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < a.npix; p += gridDim.x * kThreads) {
        const int gy = p / a.GW, gx = p - gy * a.GW;
        const float g = a.gt[gbase + p];
        bool valid = range ? (g > a.emin && g < a.emax) : (g > 0.f);
        valid = valid && gy >= a.y0 && gy < a.y1 && gx >= a.x0 && gx < a.x1;
        unsigned key = kInvalid;
        if (valid) {
            int ya, yb, xa, xb;
            double fy, fx;
            lerp_coord(gy, a.sy, a.h, ya, yb, fy);
            lerp_coord(gx, a.sx, a.w, xa, xb, fx);
            double v00 = scaled_disp<PP>(a, dbase, ya, xa), v01 = scaled_disp<PP>(a, dbase, ya, xb);
            double v10 = scaled_disp<PP>(a, dbase, yb, xa), v11 = scaled_disp<PP>(a, dbase, yb, xb);
            if (DEPTH) {
                v00 = 1.0 / v00; v01 = 1.0 / v01; v10 = 1.0 / v10; v11 = 1.0 / v11;
            }
            const double r = (1.0 - fy) * ((1.0 - fx) * v00 + fx * v01) + fy * ((1.0 - fx) * v10 + fx * v11);
            double pred;
            if (DEPTH)
                pred = a.sf * fmin(fmax(r, (double)a.emin), (double)a.emax);
            else
                pred = a.sf / r;
            key = __float_as_uint((float)pred);
            if (median && key != kInvalid) {
                const unsigned gk = __float_as_uint(g);
                atomicAdd(&lh[0 * kBins + (key >> 24)], 1u);
                atomicAdd(&lh[2 * kBins + (gk >> 24)], 1u);
            }
        }
        a.pred[gbase + p] = key;
    }
    if (median) {
        __syncthreads();
        for (int i = threadIdx.x; i < kBins; i += kThreads) {   // rank n/2 starts from the same counts
            lh[1 * kBins + i] = lh[0 * kBins + i];
            lh[3 * kBins + i] = lh[2 * kBins + i];
        }
        __syncthreads();
        const int pop = (a.flags & MD2_EVAL_POOL_BATCH) ? 0 : b;
        lds_hist_flush(lh, a.hist + (size_t)pop * kProblems * kBins);
    }
}

// grid (blocks, B): byte `shift / 8` of the keys whose higher bytes equal each problem's prefix
__global__ __launch_bounds__(kThreads) void eval_hist_kernel(EvalArgs a, int pass) {
    __shared__ unsigned lh[kProblems * kBins];
    for (int i = threadIdx.x; i < kProblems * kBins; i += kThreads) lh[i] = 0;
    const int b = blockIdx.y;
    const int pop = (a.flags & MD2_EVAL_POOL_BATCH) ? 0 : b;
    const int shift = 24 - 8 * pass;
    unsigned want[kProblems];
    bool live[kProblems];
#pragma unroll
    for (int q = 0; q < kProblems; ++q) {
        const SelState s = a.state[pop * kProblems + q];
        want[q] = s.prefix >> (shift + 8);
        live[q] = s.k != kEmpty;
    }
    __syncthreads();
    const size_t gbase = (size_t)b * a.npix;
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < a.npix; p += gridDim.x * kThreads) {
        const unsigned pk = a.pred[gbase + p];
        if (pk == kInvalid) continue;
        const unsigned gk = __float_as_uint(a.gt[gbase + p]);
#pragma unroll
        for (int q = 0; q < kProblems; ++q) {
            const unsigned key = q < 2 ? pk : gk;
            if (live[q] && (key >> (shift + 8)) == want[q]) atomicAdd(&lh[q * kBins + ((key >> shift) & 255u)], 1u);
        }
    }
    __syncthreads();
    lds_hist_flush(lh, a.hist + ((size_t)pass * a.P + pop) * kProblems * kBins);
}

// grid P * kProblems, one wave each: the bin that holds rank k, and k within it
__global__ __launch_bounds__(64) void eval_select_kernel(EvalArgs a, int pass) {
    const int pq = blockIdx.x, lane = threadIdx.x;
    const unsigned* h = a.hist + ((size_t)pass * a.P * kProblems + pq) * kBins + 4 * lane;
    const unsigned c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
    const unsigned mine = c0 + c1 + c2 + c3;
    unsigned incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    const unsigned total = __shfl(incl, 63, 64);
    SelState s = a.state[pq];
    if (pass == 0) {
        s.prefix = 0;
        s.n = total;
        s.pad = 0;
        s.k = total == 0 ? kEmpty : ((pq & 1) ? total / 2 : (total - 1) / 2);
        if (total == 0) {
            if (lane == 0) a.state[pq] = s;
            return;
        }
    } else if (s.k == kEmpty) {
        return;
    }
    const unsigned excl = incl - mine;
    if (s.k >= excl && s.k < incl) {   // exactly one lane
        unsigned k = s.k - excl, d = 0;
        if (k >= c0) { k -= c0; d = 1;
            if (k >= c1) { k -= c1; d = 2;
                if (k >= c2) { k -= c2; d = 3; } } }
        s.prefix |= (unsigned)(4 * lane + d) << (24 - 8 * pass);
        s.k = k;
        a.state[pq] = s;
    }
}

// median(gt) / median(pred) of a population; NaN when it is empty.  The medians are
// fp32 values (np.median's mean of the two middle elements is an fp32 mean); rounded to
// fp32 the fp64 quotient is the fp32 quotient (53 >= 2 * 24 + 2 bits).
__device__ __forceinline__ double eval_ratio(const EvalArgs& a, int pop) {
    if (!(a.flags & MD2_EVAL_MEDIAN_SCALE)) return 1.0;
    const SelState* s = a.state + pop * kProblems;
    if (s[0].k == kEmpty) return (double)__uint_as_float(0x7FC00000u);
    float mp = __uint_as_float(s[0].prefix), mg = __uint_as_float(s[2].prefix);
    if (!(a.flags & MD2_EVAL_MEDIAN_LOWER)) {
        mp = 0.5f * (mp + __uint_as_float(s[1].prefix));
        mg = 0.5f * (mg + __uint_as_float(s[3].prefix));
    }
    return (double)mg / (double)mp;
}

// grid (blocks, B): evaluate_depth.py:209-214 / 27-45 on the valid pixels
__global__ __launch_bounds__(kThreads) void eval_reduce_kernel(EvalArgs a) {
    const int b = blockIdx.y;
    const int pop = (a.flags & MD2_EVAL_POOL_BATCH) ? 0 : b;
    const double ratio = eval_ratio(a, pop);
    const size_t gbase = (size_t)b * a.npix;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    unsigned n1 = 0, n2 = 0, n3 = 0, n = 0;
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < a.npix; p += gridDim.x * kThreads) {
        const unsigned pk = a.pred[gbase + p];
        if (pk == kInvalid) continue;
        const double g = a.gt[gbase + p];
        double pr = (double)__uint_as_float(pk) * ratio;
        pr = pr < (double)a.emin ? (double)a.emin : pr;
        pr = pr > (double)a.emax ? (double)a.emax : pr;
        const double q = g / pr, t = fmax(q, pr / g);
        const double d = g - pr, l = log(q);
        s0 += fabs(d) / g;
        s1 += d * d / g;
        s2 += d * d;
        s3 += l * l;
        n1 += t < 1.25;
        n2 += t < 1.25 * 1.25;
        n3 += t < 1.25 * 1.25 * 1.25;
        n += 1;
    }
    __shared__ double rf[4][kThreads];
    __shared__ unsigned ru[4][kThreads];
    const int t = threadIdx.x;
    rf[0][t] = s0; rf[1][t] = s1; rf[2][t] = s2; rf[3][t] = s3;
    ru[0][t] = n1; ru[1][t] = n2; ru[2][t] = n3; ru[3][t] = n;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                rf[j][t] += rf[j][t + half];
                ru[j][t] += ru[j][t + half];
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        Partial o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o.sum[j] = rf[j][0];
            o.cnt[j] = ru[j][0];
        }
        a.part[(size_t)b * a.blocks + blockIdx.x] = o;
    }
}

// grid P, one wave: lane j < 8 sums field j of the population's partials in block order
__global__ __launch_bounds__(64) void eval_final_kernel(EvalArgs a) {
    const int pop = blockIdx.x, lane = threadIdx.x;
    const bool pool = a.flags & MD2_EVAL_POOL_BATCH;
    const int first = pool ? 0 : pop * a.blocks, count = pool ? a.B * a.blocks : a.blocks;
    double s = 0.0;
    if (lane < 8) {
        const Partial* part = a.part + first;
#pragma unroll 4
        for (int i = 0; i < count; ++i) s += lane < 4 ? part[i].sum[lane] : (double)part[i].cnt[lane - 4];
    }
    __shared__ double tot[8];
    if (lane < 8) tot[lane] = s;
    __syncthreads();
    if (lane == 0) {
        float* o = a.out + (size_t)pop * MD2_EVAL_OUT;
        const double n = tot[7];
        const float nan = __uint_as_float(0x7FC00000u);
        if (n > 0.0) {
            o[0] = (float)(tot[0] / n);
            o[1] = (float)(tot[1] / n);
            o[2] = (float)sqrt(tot[2] / n);
            o[3] = (float)sqrt(tot[3] / n);
            o[4] = (float)(tot[4] / n);
            o[5] = (float)(tot[5] / n);
            o[6] = (float)(tot[6] / n);
            o[7] = (float)eval_ratio(a, pop);
        } else {
            for (int j = 0; j < 8; ++j) o[j] = nan;
        }
        o[8] = (float)n;
        o[9] = 0.f;
    }
}

// md2_depth_export16: the `benchmark` split's export (evaluate_depth.py:148-163: cv2.resize
// of the scaled disparity to 1216 x 352, scale_factor / disp, clip, uint16(depth * 256)) for
// a batch, one launch.  grid (blocks, B); a thread owns kExportPixels adjacent pixels of one
// output row, formed as eval_predict_kernel forms its prediction (the same device functions,
// fp64 after disp_to_depth) and stored as one 8-byte word where the address allows, else as
// 4-byte words between 2-byte ends: rows of an odd width, or images at an odd offset, start
// on any 2-byte boundary.  The input is a few KB per image and stays in L2; the 2 bytes per
// pixel written are the traffic.
// This build's choice where the reference leaves the result to numpy's undefined casts: a
// resized disparity of 0 gives clip * quant (-0 and any negative one give 0), NaN gives 0.
constexpr int kExportPixels = 4;
constexpr int kMaxExportBlocks = 1024;   // per image; the rest is a grid stride

template <bool PP>
__global__ __launch_bounds__(kThreads) void export16_kernel(EvalArgs a, uint16_t* out, double clip, double quant) {
    const int b = blockIdx.y;
    const size_t dbase = (size_t)b * a.h * a.w;
    uint16_t* img = out + (size_t)b * a.npix;
    const int groups = (a.GW - 1) / kExportPixels + 1;
    const long long total = (long long)a.GH * groups;
    for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < total; g += (long long)gridDim.x * kThreads) {
        const int oy = (int)(g / groups), ox0 = (int)(g - (long long)oy * groups) * kExportPixels;
        const int n = a.GW - ox0 < kExportPixels ? a.GW - ox0 : kExportPixels;
        int ya, yb;
        double fy;
        lerp_coord(oy, a.sy, a.h, ya, yb, fy);
        unsigned q[kExportPixels];
#pragma unroll
        for (int i = 0; i < kExportPixels; ++i) {
            q[i] = 0;
            if (i < n) {
                int xa, xb;
                double fx;
                lerp_coord(ox0 + i, a.sx, a.w, xa, xb, fx);
                const double v00 = scaled_disp<PP>(a, dbase, ya, xa), v01 = scaled_disp<PP>(a, dbase, ya, xb);
                const double v10 = scaled_disp<PP>(a, dbase, yb, xa), v11 = scaled_disp<PP>(a, dbase, yb, xb);
                const double r = (1.0 - fy) * ((1.0 - fx) * v00 + fx * v01) + fy * ((1.0 - fx) * v10 + fx * v11);
                double v = a.sf / r;
                v = v > 0.0 ? (v < clip ? v : clip) : 0.0;   // NaN fails the first comparison
                q[i] = (unsigned)(v * quant);                 // <= clip * quant <= 65535
            }
        }
        uint16_t* p = img + (size_t)oy * a.GW + ox0;
        const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
        if (n == kExportPixels && (addr & 7) == 0) {
            *reinterpret_cast<uint2*>(p) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
        } else if (addr & 2) {   // one pixel up to the 4-byte boundary, a word, what is left
            p[0] = (uint16_t)q[0];
            if (n >= 3) *reinterpret_cast<unsigned*>(p + 1) = q[1] | (q[2] << 16);
            if (n == 2) p[1] = (uint16_t)q[1];
            if (n == 4) p[3] = (uint16_t)q[3];
        } else {
            if (n >= 2) *reinterpret_cast<unsigned*>(p) = q[0] | (q[1] << 16);
            if (n == 1) p[0] = (uint16_t)q[0];
            if (n == 4) *reinterpret_cast<unsigned*>(p + 2) = q[2] | (q[3] << 16);
            if (n == 3) p[2] = (uint16_t)q[2];
        }
    }
}

const char* check_export(const md2_depth16_desc* d) {
    if (!d) return "depth_export16: NULL desc";
    if (d->batch < 1 || d->in_height < 1 || d->in_width < 1 || d->out_height < 1 || d->out_width < 1)
        return "depth_export16: batch, in_height, in_width, out_height, out_width must be positive";
    if (d->batch > kMaxBatch) return "depth_export16: batch too large (at most 65535 images per call)";
    const long long in = (long long)d->in_height * d->in_width, on = (long long)d->out_height * d->out_width;
    if (in >= (1ll << 31) || on >= (1ll << 31) || d->batch * in >= (1ll << 31) || d->batch * on >= (1ll << 31))
        return "depth_export16: batch too large (2^31 pixels)";
    if (d->flags & ~MD2_DEPTH16_POST_PROCESS) return "depth_export16: unknown flags";
    if (d->reserved != 0) return "depth_export16: reserved must be 0";
    if (!(d->min_depth > 0.0) || !(d->max_depth > d->min_depth)) return "depth_export16: need 0 < min_depth < max_depth";
    const double inf = (double)INFINITY;
    if (!(d->scale_factor > 0.0) || !(d->scale_factor < inf) || !(d->clip_max > 0.0) || !(d->clip_max < inf) ||
        !(d->quant > 0.0) || !(d->quant < inf))
        return "depth_export16: scale_factor, clip_max and quant must be positive and finite";
    if (d->clip_max * d->quant > 65535.0) return "depth_export16: clip_max * quant above 65535 (the output holds 16 bits)";
    return nullptr;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Layout {
    size_t pred, hist, state, part, total;
    int P, blocks, npix;
};

const char* check_desc(const md2_eval_desc* d) {
    if (!d) return "depth_eval: NULL desc";
    if (d->batch < 1 || d->height < 1 || d->width < 1 || d->gt_height < 1 || d->gt_width < 1)
        return "depth_eval: batch, height, width, gt_height, gt_width must be positive";
    if (d->batch > kMaxBatch) return "depth_eval: batch too large (at most 65535 images per call)";
    // headroom of one grid stride below 2^31, so the pixel loops' int index cannot overflow
    if ((long long)d->batch * d->gt_height * d->gt_width >= (1ll << 31) - kMaxBlocksPerImage * kThreads ||
        (long long)d->batch * d->height * d->width >= (1ll << 31))
        return "depth_eval: batch too large (2^31 pixels)";
    if (d->crop_y0 < 0 || d->crop_x0 < 0 || d->crop_y1 > d->gt_height || d->crop_x1 > d->gt_width ||
        d->crop_y0 >= d->crop_y1 || d->crop_x0 >= d->crop_x1)
        return "depth_eval: crop must be a non-empty rectangle inside the ground-truth map";
    if (!(d->min_depth > 0.0) || !(d->max_depth > d->min_depth)) return "depth_eval: need 0 < min_depth < max_depth";
    if (!(d->eval_min > 0.f) || !(d->eval_max > d->eval_min)) return "depth_eval: need 0 < eval_min < eval_max";
    if (!(d->scale_factor > 0.0) || !(d->scale_factor < (double)INFINITY)) return "depth_eval: scale_factor must be positive";
    return nullptr;
}

Layout layout(const md2_eval_desc* d) {
    Layout l;
    l.npix = d->gt_height * d->gt_width;
    l.P = (d->flags & MD2_EVAL_POOL_BATCH) ? 1 : d->batch;
    const int want = (l.npix + kThreads * kPixelsPerThread - 1) / (kThreads * kPixelsPerThread);
    l.blocks = want < 1 ? 1 : (want > kMaxBlocksPerImage ? kMaxBlocksPerImage : want);
    size_t off = 0;
    l.pred = off;  off += align256(sizeof(unsigned) * (size_t)d->batch * l.npix);
    l.hist = off;  off += align256(sizeof(unsigned) * (size_t)kPasses * l.P * kProblems * kBins);
    l.state = off; off += align256(sizeof(SelState) * (size_t)l.P * kProblems);
    l.part = off;  off += align256(sizeof(Partial) * (size_t)d->batch * l.blocks);
    l.total = off;
    return l;
}

}  // namespace

extern "C" {

size_t md2_depth_eval_workspace_bytes(const md2_eval_desc* d) {
    if (const char* msg = check_desc(d)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return layout(d).total;
}

int md2_depth_eval(const md2_eval_desc* d, const float* disp, const float* disp_flipped, const float* gt,
                   float* out, void* workspace, void* stream) {
    if (const char* msg = check_desc(d)) return md2_report_error(MD2_ERR_ARG, msg);
    if (!disp || !gt || !out || !workspace) return md2_report_error(MD2_ERR_ARG, "depth_eval: NULL operand");
    const bool pp = d->flags & MD2_EVAL_POST_PROCESS, depth = d->flags & MD2_EVAL_RESIZE_DEPTH;
    if (pp && !disp_flipped)
        return md2_report_error(MD2_ERR_ARG, "depth_eval: MD2_EVAL_POST_PROCESS needs disp_flipped");
    const Layout l = layout(d);
    char* ws = static_cast<char*>(workspace);
    EvalArgs a = {};
    a.disp = disp;
    a.dispf = disp_flipped;
    a.gt = gt;
    a.pred = reinterpret_cast<unsigned*>(ws + l.pred);
    a.hist = reinterpret_cast<unsigned*>(ws + l.hist);
    a.state = reinterpret_cast<SelState*>(ws + l.state);
    a.part = reinterpret_cast<Partial*>(ws + l.part);
    a.out = out;
    a.B = d->batch; a.h = d->height; a.w = d->width; a.GH = d->gt_height; a.GW = d->gt_width;
    a.npix = l.npix; a.P = l.P; a.blocks = l.blocks;
    a.y0 = d->crop_y0; a.y1 = d->crop_y1; a.x0 = d->crop_x0; a.x1 = d->crop_x1;
    a.flags = d->flags;
    // torch's disp_to_depth: min_disp + (max_disp - min_disp) * disp with the two Python
    // doubles 1 / max_depth and 1 / min_depth, each scalar operand rounded to fp32
    const double lo = 1.0 / d->max_depth, hi = 1.0 / d->min_depth;
    a.lo = (float)lo;
    a.range = (float)(hi - lo);
    a.emin = d->eval_min; a.emax = d->eval_max; a.sf = d->scale_factor;
    a.sy = (double)d->height / (double)d->gt_height;
    a.sx = (double)d->width / (double)d->gt_width;

    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(l.blocks, d->batch), block(kThreads);
    const bool median = d->flags & MD2_EVAL_MEDIAN_SCALE;
    if (median) {
        const hipError_t e = hipMemsetAsync(a.hist, 0, sizeof(unsigned) * (size_t)kPasses * l.P * kProblems * kBins, st);
        if (e != hipSuccess) return md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
    }
    auto predict = pp ? (depth ? eval_predict_kernel<true, true> : eval_predict_kernel<true, false>)
                      : (depth ? eval_predict_kernel<false, true> : eval_predict_kernel<false, false>);
    hipLaunchKernelGGL(predict, grid, block, 0, st, a);
    if (median) {
        for (int pass = 0; pass < kPasses; ++pass) {
            if (pass > 0) hipLaunchKernelGGL(eval_hist_kernel, grid, block, 0, st, a, pass);
            hipLaunchKernelGGL(eval_select_kernel, dim3(l.P * kProblems), dim3(64), 0, st, a, pass);
        }
    }
    hipLaunchKernelGGL(eval_reduce_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(eval_final_kernel, dim3(l.P), dim3(64), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

int md2_depth_export16_check(const md2_depth16_desc* d) {
    if (const char* msg = check_export(d)) return md2_report_error(MD2_ERR_ARG, msg);
    return MD2_OK;
}

int md2_depth_export16(const md2_depth16_desc* d, const float* disp, const float* disp_flipped, uint16_t* out,
                       void* stream) {
    if (const char* msg = check_export(d)) return md2_report_error(MD2_ERR_ARG, msg);
    if (!disp || !out) return md2_report_error(MD2_ERR_ARG, "depth_export16: NULL operand");
    const bool pp = d->flags & MD2_DEPTH16_POST_PROCESS;
    if (pp && !disp_flipped)
        return md2_report_error(MD2_ERR_ARG, "depth_export16: MD2_DEPTH16_POST_PROCESS needs disp_flipped");
    if (reinterpret_cast<uintptr_t>(out) & 1) return md2_report_error(MD2_ERR_ARG, "depth_export16: out must be 2-byte aligned");
    EvalArgs a = {};
    a.disp = disp;
    a.dispf = disp_flipped;
    a.B = d->batch; a.h = d->in_height; a.w = d->in_width; a.GH = d->out_height; a.GW = d->out_width;
    a.npix = d->out_height * d->out_width;
    const double lo = 1.0 / d->max_depth, hi = 1.0 / d->min_depth;   // as md2_depth_eval
    a.lo = (float)lo;
    a.range = (float)(hi - lo);
    a.sf = d->scale_factor;
    a.sy = (double)d->in_height / (double)d->out_height;
    a.sx = (double)d->in_width / (double)d->out_width;
    const long long groups = (long long)d->out_height * ((d->out_width - 1) / kExportPixels + 1);
    const long long want = (groups + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(want > kMaxExportBlocks ? kMaxExportBlocks : want), d->batch), block(kThreads);
    hipLaunchKernelGGL(pp ? export16_kernel<true> : export16_kernel<false>, grid, block, 0, (hipStream_t)stream, a, out,
                       d->clip_max, d->quant);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
