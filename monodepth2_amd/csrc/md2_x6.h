// md2_x6.h — the split-bf16 ("x6") operand format, shared by conv.hip, direct.hip and
// stem.hip.  This header is its one definition:
//   - the split: every f32 operand is cut exactly into three bf16 planes by truncation,
//     x == x0 + x1 + x2 (8 + 8 + 8 significand bits);
//   - the layout: operands sit in LDS planes [row][32 k] bf16 whose 16-byte quads are
//     XOR-swizzled (xidx / xidx2 / xsw);
//   - the product: the six terms xi*yj with i + j <= 2, accumulated small terms first
//     (x6_mma32 / x6_mma16); the one-plane (bf16 operand) form is their NP = 1 case.
// Kernels that agree bitwise (tests/test_conv_gpu.py) do so because they all go through
// these functions.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "md2_bf16.h"

namespace md2 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------- the split
// Exact three-way split by truncation: x0 = x with the low 16 bits cleared (the top 8
// significand bits), r1 = x - x0 exact (<= 16 significant bits), x1 = r1 truncated the
// same way, x2 = r1 - x1 exact with <= 8 significant bits, so its bf16 (the high half)
// is exact too: x == x0 + x1 + x2.  Pairs of elements are packed with one v_perm per
// plane (the high halves of two dwords).
__device__ __forceinline__ float trunc16(float x) {
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, x) & 0xFFFF0000u);
}
__device__ __forceinline__ uint32_t hi16x2(float lo, float hi) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, hi), __builtin_bit_cast(uint32_t, lo), 0x07060302u);
}
// component j (a compile-time constant after unrolling) of a float4
__device__ __forceinline__ float chan(float4 v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); }
// one scalar: the three planes as f32 values (bf16 = their high halves)
__device__ __forceinline__ void split3(float x, float& x0, float& x1, float& x2) {
    x0 = trunc16(x);
    const float r1 = x - x0;
    x1 = trunc16(r1);
    x2 = r1 - x1;
}
// one scalar to element i of three planes of n bf16 each
__device__ __forceinline__ void split_store(__bf16* out, int n, int i, float v) {
    float a, b, c;
    split3(v, a, b, c);
    out[i] = __builtin_bit_cast(__bf16, (uint16_t)(__builtin_bit_cast(uint32_t, a) >> 16));
    out[n + i] = __builtin_bit_cast(__bf16, (uint16_t)(__builtin_bit_cast(uint32_t, b) >> 16));
    out[2 * n + i] = __builtin_bit_cast(__bf16, (uint16_t)(__builtin_bit_cast(uint32_t, c) >> 16));
}
// four consecutive k of one row
__device__ __forceinline__ void split3(float4 v, bf16x4& p0, bf16x4& p1, bf16x4& p2) {
    const float x[4] = {v.x, v.y, v.z, v.w};
    float a[4], b[4], c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split3(x[i], a[i], b[i], c[i]);
    u32x2 q0, q1, q2;
    q0.x = hi16x2(a[0], a[1]), q0.y = hi16x2(a[2], a[3]);
    q1.x = hi16x2(b[0], b[1]), q1.y = hi16x2(b[2], b[3]);
    q2.x = hi16x2(c[0], c[1]), q2.y = hi16x2(c[2], c[3]);
    p0 = __builtin_bit_cast(bf16x4, q0);
    p1 = __builtin_bit_cast(bf16x4, q1);
    p2 = __builtin_bit_cast(bf16x4, q2);
}
// Transposing micro-tile: v[i] holds channels j = 0..3 of k (pixel) i = 0..3.  Channel j's
// four consecutive k leave as one 8-byte run per plane, (k0k1, k2k3) packed bf16 pairs:
// run(pl, j, k0k1, k2k3) is called once per plane and channel.
template <typename F>
__device__ __forceinline__ void split4x4_runs(const float4* v, F&& run) {
    float c[3][4][4];   // plane, k i, channel j
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) split3(x[j], c[0][i][j], c[1][i][j], c[2][i][j]);
    }
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int j = 0; j < 4; ++j) run(pl, j, hi16x2(c[pl][0][j], c[pl][1][j]), hi16x2(c[pl][2][j], c[pl][3][j]));
}
// its one-plane case: bf16 operands (four channels in a uint2), repacked, not split.
// Channel j of two k: the low / high halves of dword j / 2 of each
__device__ __forceinline__ uint32_t pair16(uint2 k0, uint2 k1, int j) {
    return __builtin_amdgcn_perm(j < 2 ? k1.x : k1.y, j < 2 ? k0.x : k0.y, (j & 1) ? 0x07060302u : 0x05040100u);
}
template <typename F>
__device__ __forceinline__ void split4x4_runs(const uint2* v, F&& run) {
#pragma unroll
    for (int j = 0; j < 4; ++j) run(0, j, pair16(v[0], v[1], j), pair16(v[2], v[3], j));
}
// ... into pk[plane][channel j][(k0k1, k2k3)]
template <typename V, int NP>
__device__ __forceinline__ void split4x4(const V* v, uint32_t (&pk)[NP][4][2]) {
    split4x4_runs(v, [&](int pl, int j, uint32_t lo, uint32_t hi) {
        pk[pl][j][0] = lo;
        pk[pl][j][1] = hi;
    });
}

// ---------------------------------------------------------------- the layout
constexpr int XBK = 32;   // k per LDS row (one K chunk)

// element index of (row r, k) in a [rows][32] bf16 plane, 16-byte quads swizzled
__device__ __forceinline__ int xidx(int r, int k) { return r * XBK + ((((k >> 3) ^ (r >> 2)) & 3) << 3) + (k & 7); }
// xidx with rows r and r ^ 1 swapped in every odd row quad: the same ds_read_b128
// banks as xidx (a fragment group's rows map onto the same row set), and an 8-byte
// store of row 4 q + j by the 16 lanes of two quads (q, q + 1) then lands on both
// 16-bank halves (row parity differs) instead of two-way on one
__device__ __forceinline__ int xidx2(int r, int k) { return xidx(r ^ ((r >> 2) & 1), k); }
// The 16x16x32 MFMA path's operand layout: k-octet slot kq ^ (row >> 2 & 2).  Its
// ds_read_b128 lane groups ({0-3, 12-15, 20-27}, ...) read rows c, 12 + c at one octet
// and 4 + c, 8 + c at the next, which xidx's kq ^ (row >> 2) puts on the same 16-byte
// bank slot (two-way on every fragment read); this slot function keeps all four apart.
template <int MT>
__device__ __forceinline__ int xsw(int r, int k) {
    if constexpr (MT == 32) return xidx(r, k);
    return r * XBK + ((((k >> 3) ^ ((r >> 2) & 2)) & 3) << 3) + (k & 7);
}

// Workgroup barrier that leaves LDS-DMA loads in flight: __syncthreads()'s fence
// would wait for every outstanding vector-memory op (vmcnt(0)) once LDS-DMA is in
// the kernel, draining the register prefetch of A; the DMA is ordered by explicit
// wait_vm<> calls instead.  The "memory" clobber keeps LDS accesses on their side.
__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int VM>
__device__ __forceinline__ void wait_vm() {
    static_assert(VM >= 0 && VM < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt((VM & 0xF) | ((VM >> 4) << 14) | (0x7 << 4) | (0xF << 8));
}

// Workgroups are dealt round-robin over the 8 XCDs (bid & 7; speed only, never
// correctness).  The logical block of hardware block `bid` of n such that every XCD runs
// a contiguous range of logical blocks: its private L2 then streams a contiguous slice
// of the operands instead of all XCDs fetching everything.  Bijective for any n.
__device__ __forceinline__ int xcd_contiguous_block(int bid, int n) {
    const int q = n >> 3, r = n & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    return xcd < r ? xcd * (q + 1) + idx : r * (q + 1) + (xcd - r) * q + idx;
}

// ---------------------------------------------------------------- the product
// acc + x * y on NP planes per operand.  NP = 3: the six products with i + j <= 2 (the
// three dropped ones are below 2^-24 relative), small terms first: x2y0, x1y1, x0y2,
// x1y0, x0y1, x0y0.  NP = 1: bf16 operands, the one product.
template <int NP, typename Acc>
__device__ __forceinline__ Acc x6_mma32(const bf16x8 (&x)[NP], const bf16x8 (&y)[NP], Acc acc) {
    static_assert(NP == 1 || NP == 3, "planes per operand");
    if constexpr (NP == 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[2], y[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1], y[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1], y[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[1], acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[0], acc, 0, 0, 0);
}
template <int NP, typename Acc>
__device__ __forceinline__ Acc x6_mma16(const bf16x8 (&x)[NP], const bf16x8 (&y)[NP], Acc acc) {
    static_assert(NP == 1 || NP == 3, "planes per operand");
    if constexpr (NP == 3) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[2], y[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[1], y[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[0], y[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[1], y[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[0], y[1], acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[0], y[0], acc, 0, 0, 0);
}

}  // namespace md2
