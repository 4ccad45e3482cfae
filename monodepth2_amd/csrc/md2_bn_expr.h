// md2_bn_expr.h — the per-element expressions of the BatchNorm / ReLU / max-pool passes,
// shared by the kernels that run them as passes of their own (bnorm.hip, pool.hip) and
// by the kernels that fold such a pass into a neighbour (the stem's fused
// BatchNorm + ReLU + max-pool forward in bnorm.hip, stem.hip's weight gradient that
// forms the BatchNorm input gradient on load).  One source for both, so a folded pass
// gives the bits of the pass it replaces.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace md2 {

// bn_apply: (x - mean)·invstd·γ + β
__device__ __forceinline__ float4 bn_affine4(const float4 v, const float4 mu, const float4 is, const float4 ga,
                                             const float4 be) {
    float4 o;
    o.x = (v.x - mu.x) * is.x * ga.x + be.x;
    o.y = (v.y - mu.y) * is.y * ga.y + be.y;
    o.z = (v.z - mu.z) * is.z * ga.z + be.z;
    o.w = (v.w - mu.w) * is.w * ga.w + be.w;
    return o;
}

__device__ __forceinline__ float4 relu4(float4 o) {
    o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
    return o;
}

// the backward's ReLU gate from the forward's mask byte (bit i = y[4 q + i] > 0); off is
// the element offset of the quad
__device__ __forceinline__ float4 relu_gate_bits4(const uint32_t m, float4 g) {
    g.x = (m & 1) ? g.x : 0.f; g.y = (m & 2) ? g.y : 0.f; g.z = (m & 4) ? g.z : 0.f; g.w = (m & 8) ? g.w : 0.f;
    return g;
}
__device__ __forceinline__ float4 relu_gate_mask4(const void* mask, size_t off, float4 g) {
    return relu_gate_bits4(((const uint8_t*)mask)[off >> 2], g);
}

// bn_bwd_apply: dx = k1·(g' - k2 - (x - mean)·k3) with bn_bwd_final's coefficient rows
// k1 = γ·invstd, k2 = Σg'/N, k3 = Σg'x̂/N · invstd
__device__ __forceinline__ float4 bn_bwd_dx4(const float4 gv, const float4 v, const float4 mu, const float4 k1,
                                             const float4 k2, const float4 k3) {
    float4 o;
    o.x = k1.x * (gv.x - k2.x - (v.x - mu.x) * k3.x);
    o.y = k1.y * (gv.y - k2.y - (v.y - mu.y) * k3.y);
    o.z = k1.z * (gv.z - k2.z - (v.z - mu.z) * k3.z);
    o.w = k1.w * (gv.w - k2.w - (v.w - mu.w) * k3.w);
    return o;
}

// one window tap of the max-pool (ATen max_pool2d: strictly greater, or NaN)
__device__ __forceinline__ void pool_take(float v, int k, float& m, int& a) {
    if (v > m || isnan(v)) {
        m = v;
        a = k;
    }
}

}  // namespace md2
