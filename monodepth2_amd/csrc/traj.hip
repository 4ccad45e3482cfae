// traj.hip — KITTI odometry pose evaluation (absolute trajectory error) on gfx950.
//
// Reference: evaluate_pose.py:104-125.  It turns the ground truth's global poses into
// local ones with two LAPACK inverses per frame, then for every frame chains up to
// track_length - 1 predicted and ground-truth transforms into two little trajectories
// (dump_xyz), aligns them by one least-squares scale (compute_ate) and reports the mean
// and the standard deviation of the errors — on the host, in a Python loop.  Here
// (md2_pose_ate, include/md2hot.h) a batch of sequences is a fixed chain of three
// launches, every step in fp64:
//
//   local     one thread per frame pair, the sequence on grid.y:
//             L_i = inv(inv(G_{i-1}) . G_i) into the workspace (each inverted once)
//   ate       one thread per snippet: both trajectories, scale, rmse -> ates
//   stats     one block per sequence: mean and population std of its ates through a
//             reduction of fixed shape (256 lanes striding in rising order, then a
//             halving tree) — no atomics, independent of the launch geometry
//
// Arithmetic: every product and sum is a separately rounded fp64 operation in the written
// order (no contraction), so tests/pose_eval_case.py can restate it in numpy bit for bit.
// The inverse is the general affine one (cofactors over the determinant, then -A^-1 t),
// not [R^T | -R^T t]: KITTI's pose files carry seven digits, their rotations are
// orthonormal to 1e-7 only, and hundreds of metres from the origin the shortcut moves the
// error by 1e-7..1e-6 relative, where this agrees with LAPACK to about 1e-12.
// Matrix products are the plain four-term sums ((a0*b0 + a1*b1) + a2*b2) + a3*b3 with the
// bottom row present: [0,0,0,1] for the ground truth, the stored row for a prediction.

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "md2hot.h"

int md2_report_error(int code, const char* msg);

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSequences = 65535;   // sequences are grid.y
constexpr int kMaxBlocks = 1024;       // per sequence; longer sequences stride
constexpr int kMaxTrack = 16;

struct TrajArgs {
    const float* pred;
    const double* gt;
    const long long* offsets;
    double* local;      // (total - S, 3, 4)
    double* ates;       // (total - S)
    double* stats;      // (S, 2)
    long long total;
    long long rows;     // total - S
    int S, track;
};

// The frames [begin, end) of sequence s and the first row of its transforms and errors.
// The contract is 0 = o[0] <= ... <= o[S] = total with o[s+1] - o[s] >= 2; the clamps and
// the row test keep a broken table from touching anything outside the operands (what it
// then computes is meaningless).
struct Span {
    long long begin, row0, pairs;   // pairs = M_s - 1, <= 0 for a short sequence
};

__device__ __forceinline__ Span span_of(const TrajArgs& a, int s) {
    long long begin = a.offsets[s], end = a.offsets[s + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > a.total ? a.total : end;
    Span sp;
    sp.begin = begin;
    sp.row0 = begin - s;
    sp.pairs = end - begin - 1;
    if (sp.row0 < 0 || sp.row0 + sp.pairs > a.rows) sp.pairs = 0;
    return sp;
}

// inverse of the affine [A | t; 0 0 0 1], 3x4 row-major -> 3x4
__device__ __forceinline__ void affine_inverse(const double* m, double* o) {
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], k = m[10];
    const double c00 = e * k - f * h, c01 = f * g - d * k, c02 = d * h - e * g;
    const double c10 = c * h - b * k, c11 = a * k - c * g, c12 = b * g - a * h;
    const double c20 = b * f - c * e, c21 = c * d - a * f, c22 = a * e - b * d;
    const double det = (a * c00 + b * c01) + c * c02;
    o[0] = c00 / det; o[1] = c10 / det; o[2] = c20 / det;
    o[4] = c01 / det; o[5] = c11 / det; o[6] = c21 / det;
    o[8] = c02 / det; o[9] = c12 / det; o[10] = c22 / det;
    const double x = m[3], y = m[7], z = m[11];
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r * 4 + 3] = -((o[r * 4] * x + o[r * 4 + 1] * y) + o[r * 4 + 2] * z);
}

// top three rows of A . B; A 3x4 (its bottom row does not enter them), B 4x4
__device__ __forceinline__ void mul34(const double* A, const double* B, double* C) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            C[r * 4 + c] = ((A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c]) + A[r * 4 + 2] * B[8 + c]) + A[r * 4 + 3] * B[12 + c];
    }
}

__device__ __forceinline__ void bottom_row(double* M) {
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
}

// grid (blocks, S)
__global__ __launch_bounds__(kThreads) void traj_local_kernel(TrajArgs a) {
    const int s = blockIdx.y;
    const Span sp = span_of(a, s);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < sp.pairs;
         i += (long long)gridDim.x * kThreads) {
        const double* g = a.gt + (size_t)(sp.begin + i) * 12;
        double G0[12], G1[16], inv0[12], rel[12], out[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) { G0[j] = g[j]; G1[j] = g[12 + j]; }
        bottom_row(G1);
        affine_inverse(G0, inv0);
        mul34(inv0, G1, rel);
        affine_inverse(rel, out);
        double* dst = a.local + (size_t)(sp.row0 + i) * 12;
#pragma unroll
        for (int j = 0; j < 12; ++j) dst[j] = out[j];
    }
}

// grid (blocks, S)
__global__ __launch_bounds__(kThreads) void traj_ate_kernel(TrajArgs a) {
    const int s = blockIdx.y;
    const Span sp = span_of(a, s);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < sp.pairs;
         i += (long long)gridDim.x * kThreads) {
        long long n = sp.pairs - i;                       // the reference's slice truncation
        n = n > a.track - 1 ? a.track - 1 : n;
        double gp[kMaxTrack][3], pp[kMaxTrack][3];
        double Cg[12], Cp[12], T[16], N[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) Cg[j] = Cp[j] = (j % 5 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) gp[0][c] = pp[0][c] = 0.0;
        for (int k = 0; k < (int)n; ++k) {
            const double* l = a.local + (size_t)(sp.row0 + i + k) * 12;
#pragma unroll
            for (int j = 0; j < 12; ++j) T[j] = l[j];
            bottom_row(T);
            mul34(Cg, T, N);
#pragma unroll
            for (int j = 0; j < 12; ++j) Cg[j] = N[j];
            const float* p = a.pred + (size_t)(sp.row0 + i + k) * 16;
#pragma unroll
            for (int j = 0; j < 16; ++j) T[j] = (double)p[j];
            mul34(Cp, T, N);
#pragma unroll
            for (int j = 0; j < 12; ++j) Cp[j] = N[j];
#pragma unroll
            for (int c = 0; c < 3; ++c) { gp[k + 1][c] = Cg[c * 4 + 3]; pp[k + 1][c] = Cp[c * 4 + 3]; }
        }
        // compute_ate (evaluate_pose.py:34-46); the offset is 0 - 0, kept as written
        double off[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) off[c] = gp[0][c] - pp[0][c];
        double num = 0.0, den = 0.0;
        for (int k = 0; k <= (int)n; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double p = pp[k][c] + off[c];
                pp[k][c] = p;
                num = num + gp[k][c] * p;
                den = den + p * p;
            }
        }
        const double scale = num / den;
        double sse = 0.0;
        for (int k = 0; k <= (int)n; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double e = pp[k][c] * scale - gp[k][c];
                sse = sse + e * e;
            }
        }
        a.ates[sp.row0 + i] = sqrt(sse) / (double)(n + 1);
    }
}

// lane t's strided sum of f(x[t]), f(x[t + 256]), ... folded by a halving tree; all lanes
// must call it; the result is valid in every lane
template <bool kDeviation>
__device__ __forceinline__ double block_sum(const double* x, long long count, double mean, double* lds) {
    const int t = threadIdx.x;
    double acc = 0.0;
    for (long long j = t; j < count; j += kThreads) {
        double v = x[j];
        if (kDeviation) {
            const double dv = v - mean;
            v = dv * dv;
        }
        acc = acc + v;
    }
    __syncthreads();          // the previous call's readers are done with lds
    lds[t] = acc;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (t < half) lds[t] = lds[t] + lds[t + half];
        __syncthreads();
    }
    return lds[0];
}

// grid (S), 256 threads
__global__ __launch_bounds__(kThreads) void traj_stats_kernel(TrajArgs a) {
    __shared__ double lds[kThreads];
    const int s = blockIdx.x;
    const Span sp = span_of(a, s);
    double* out = a.stats + (size_t)s * 2;
    if (sp.pairs < 1) {       // shorter than two frames (or a broken table): nan, block-uniform
        if (threadIdx.x == 0) out[0] = out[1] = __builtin_nan("");
        return;
    }
    const double* x = a.ates + sp.row0;
    const double cnt = (double)sp.pairs;
    const double mean = block_sum<false>(x, sp.pairs, 0.0, lds) / cnt;
    const double var = block_sum<true>(x, sp.pairs, mean, lds) / cnt;
    if (threadIdx.x == 0) {
        out[0] = mean;
        out[1] = sqrt(var);
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

const char* check_desc(const md2_pose_ate_desc* d) {
    if (!d) return "pose_ate: NULL desc";
    if (d->sequences < 1) return "pose_ate: sequences must be at least 1";
    if (d->track_length < 2 || d->track_length > kMaxTrack) return "pose_ate: track_length must be 2..16";
    if (d->flags) return "pose_ate: unknown flags (none are defined)";
    if (d->total_frames < 2 * (int64_t)d->sequences)
        return "pose_ate: total_frames below 2 * sequences (every sequence needs two frames)";
    if (d->sequences > kMaxSequences) return "pose_ate: too many sequences (at most 65535 per call)";
    if (d->total_frames >= (1ll << 31)) return "pose_ate: too many frames (2^31)";
    return nullptr;
}

}  // namespace

extern "C" {

size_t md2_pose_ate_workspace_bytes(const md2_pose_ate_desc* d) {
    if (const char* msg = check_desc(d)) {
        md2_report_error(MD2_ERR_ARG, msg);
        return 0;
    }
    return align256(sizeof(double) * 12 * (size_t)(d->total_frames - d->sequences));
}

int md2_pose_ate(const md2_pose_ate_desc* d, const float* pred, const double* gt, const int64_t* offsets,
                 double* ates, double* stats, void* workspace, void* stream) {
    if (const char* msg = check_desc(d)) return md2_report_error(MD2_ERR_ARG, msg);
    if (!pred || !gt || !offsets || !ates || !stats || !workspace)
        return md2_report_error(MD2_ERR_ARG, "pose_ate: NULL operand");
    if (reinterpret_cast<uintptr_t>(workspace) % 256)
        return md2_report_error(MD2_ERR_ARG, "pose_ate: workspace must be 256-byte aligned");
    TrajArgs a = {};
    a.pred = pred;
    a.gt = gt;
    a.offsets = reinterpret_cast<const long long*>(offsets);
    a.local = static_cast<double*>(workspace);
    a.ates = ates;
    a.stats = stats;
    a.total = d->total_frames;
    a.rows = d->total_frames - d->sequences;
    a.S = d->sequences;
    a.track = d->track_length;

    const hipStream_t st = (hipStream_t)stream;
    // the mean sequence's worth of threads per sequence; a longer one strides
    const long long mean = (a.rows + a.S - 1) / a.S;
    long long blocks = (mean + kThreads - 1) / kThreads;
    blocks = blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks);
    const dim3 grid((unsigned)blocks, (unsigned)a.S);
    hipLaunchKernelGGL(traj_local_kernel, grid, dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(traj_ate_kernel, grid, dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(traj_stats_kernel, dim3((unsigned)a.S), dim3(kThreads), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MD2_OK : md2_report_error(MD2_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
