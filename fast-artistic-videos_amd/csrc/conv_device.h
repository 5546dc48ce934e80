// Device-side pieces shared by the convolution kernels (kernels_conv / c8 / halo / halo_s2 / fold / elem / wino / up2 / s2 / first):
// vector types, tile constants and small force-inlined helpers.
#pragma once
#include "fav_internal.h"

namespace fav {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));   // native vector: struct float4 copies lower to memcpy through scratch
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int BM = CONV_BM;   // 128 output pixels per block
constexpr int BK = 32;        // K elements per step
constexpr int LDSS = 36;      // LDS row stride in floats (144 B: 16-B aligned, conflict-free b128 reads)
constexpr int SK_GRID = 512;            // stream-K grid: 2 blocks on each of the 256 CUs, all co-resident

// XCD-aware block order: the dispatcher places block b on XCD b % 8 (observed; used for L2 locality only).
// Give every XCD a contiguous range of logical blocks so the halo rows of neighbouring tiles hit its L2
// (and stream-K hand-offs mostly stay inside one XCD).  Returns the logical index of this block.
__device__ __forceinline__ int xcd_linear_block()
{
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// 16-byte write-through store (sc1): the stream-K partial tiles are published with these + `s_waitcnt vmcnt(0)` + an sc1 flag
// store, instead of plain stores + an agent-scope release fence (which writes back the whole XCD L2's dirty lines, i.e. also the
// output tiles other blocks are storing at that moment): MI355X_MICROARCH.md "publish-large" row, 8.2 -> 3.0 us per 64 KB.
__device__ __forceinline__ void store16_wt(void* p, v4f v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}

// Per-tile InstanceNorm partials with ONE barrier: every wave reduces its own 32 pixels x 32 channels accumulator tile(s) to
// (mean, M2, count) in registers (two half-wave shuffles), the NW waves' results meet in LDS, and thread c merges the waves of
// channel c exactly (Chan et al.): mean = sum n_w mean_w / n, M2 = sum M2_w + n_w (mean_w - mean)^2.  (Before: block-wide
// sum -> barrier -> mean -> barrier -> M2 -> barrier -> barrier, four barriers per tile on an 8-wave block.)
__device__ __forceinline__ float2 merge_wave_stats(const float2* st, const int* wn, int NW, int pitch, int c, int* n_out)
{
    int n = 0; float s = 0.f;
    for (int w = 0; w < NW; ++w) { n += wn[w]; s += (float)wn[w] * st[w * pitch + c].x; }
    const float mean = n ? s / (float)n : 0.f;
    float m2 = 0.f;
    for (int w = 0; w < NW; ++w) { const float d = st[w * pitch + c].x - mean; m2 += st[w * pitch + c].y + (float)wn[w] * d * d; }
    *n_out = n;
    return make_float2(mean, m2);
}

// branch-free form used inside the MFMA loop: lo = 0 for ReLU, -inf for none; identity = scale 1, shift 0
__device__ __forceinline__ float4 affine4_lo(float4 v, const float* sc, const float* sh, float lo)
{
    const float4 s = *reinterpret_cast<const float4*>(sc);
    const float4 b = *reinterpret_cast<const float4*>(sh);
    v.x = fmaxf(fmaf(v.x, s.x, b.x), lo); v.y = fmaxf(fmaf(v.y, s.y, b.y), lo);
    v.z = fmaxf(fmaf(v.z, s.z, b.z), lo); v.w = fmaxf(fmaf(v.w, s.w, b.w), lo);
    return v;
}

__device__ __forceinline__ float4 affine4(float4 v, const float* sc, const float* sh, int relu)
{
    const float4 s = *reinterpret_cast<const float4*>(sc);
    const float4 b = *reinterpret_cast<const float4*>(sh);
    v.x = fmaf(v.x, s.x, b.x); v.y = fmaf(v.y, s.y, b.y); v.z = fmaf(v.z, s.z, b.z); v.w = fmaf(v.w, s.w, b.w);
    if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    return v;
}

}  // namespace fav
