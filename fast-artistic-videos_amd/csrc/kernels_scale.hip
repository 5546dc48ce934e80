// kernels_scale.hip -- -scale_factor for gfx950: image.scale(src, Wd, Hd, 'bicubic') on float tensors [Torch7 `image`, recalled: the
// package is not vendored] around the frames that have no prior (fast_artistic_video_core.lua:127-130,150-152).
//
// The scaling is separable: along the WIDTH first, into an fp32 intermediate [C][Hs][Wd], then along the height.  Along one axis
// (src_len source samples s, dst_len destination samples d):
//   dst_len == src_len         d = s
//   src_len == 1               d[*] = s[0]
//   otherwise                  scale = (float)(src_len - 1) / (float)(dst_len - 1); for di < dst_len - 1:
//                                f = di * scale, i = (long)f, x = f - i, p1 = s[i], p2 = s[i + 1],
//                                p0 = i > 0 ? s[i - 1] : 2 p1 - p2,  p3 = i + 2 < src_len ? s[i + 2] : 2 p2 - p1,
//                                d[di] = p1 + 0.5 x (p2 - p0 + x (2 p0 - 5 p1 + 4 p2 - p3 + x (3 (p1 - p2) + p3 - p0)))
//                              and d[dst_len - 1] = s[src_len - 1]
// No clamping, no antialiasing; the same formula serves factors below and above 1.
//
// Neither kernel materialises the intermediate: a destination sample forms the (up to) four width-pass values it needs -- each rounded
// to fp32, the height pass's border extrapolation acting on THEM -- and combines them.  Both are memory-bound gathers, one lane per
// destination sample and consecutive lanes on consecutive x: a wave's 4 x 4 neighbourhoods overlap into (at most) four dense source row
// segments that the vector L1 / L2 serve, every source line leaves HBM once, and the stores are dense 16-byte ones.  (Staging source
// tiles in LDS would save load instructions, not traffic: at 3840x2160 -> 1920x1080 the pair is a small fraction of the network it brackets,
// DESIGN.md section 4.)
// Compiled with -ffp-contract=off so that every operation rounds like the CPU restatement (tests/util/bicubic_model.py).
#include "cubic.h"
#include "fav_internal.h"

namespace fav {
namespace {

__device__ __forceinline__ int reflect(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// where destination sample di of an axis comes from: s[i] itself (cubic == 0: equal lengths, a one-sample source, the last sample) or
// the cubic through s[i - 1 .. i + 2] at x
struct AxisTap { int i; float x; int cubic; };

__device__ __forceinline__ AxisTap axis_tap(int di, int src_len, int dst_len, float scale)
{
    AxisTap t; t.x = 0.f; t.cubic = 0;
    if (dst_len == src_len) { t.i = di; return t; }
    if (src_len == 1) { t.i = 0; return t; }
    if (di == dst_len - 1) { t.i = src_len - 1; return t; }
    const float f = (float)di * scale;
    t.i = min((int)f, src_len - 2);      // (never the smaller one for a rounded scale: f < src_len - 1 by (src_len - 1) / (dst_len - 1); keeps s[i + 1] addressable)
    t.x = f - (float)t.i;
    t.cubic = 1;
    return t;
}

template <class Sample>
__device__ __forceinline__ float resample(const AxisTap& t, int src_len, Sample s)
{
    if (!t.cubic) return s(t.i);
    const float p1 = s(t.i), p2 = s(t.i + 1);
    const float p0 = t.i > 0 ? s(t.i - 1) : 2.f * p1 - p2;
    const float p3 = t.i + 2 < src_len ? s(t.i + 2) : 2.f * p2 - p1;
    return catmull_rom(p0, p1, p2, p3, t.x);
}

// scale_prep: the first frame's network input at the scaled size in one launch -- image.load's byte / 255, the resampling H x W ->
// Hs x Ws, vgg.preprocess, the fill / zero prior and mask planes and the folded reflection padding -> padded NHWC8 [Hs+2p][Ws+2p][8].
// With Hs x Ws == H x W this writes what prep_input_kernel writes for a frame without a prior.
__global__ __launch_bounds__(256) void scale_prep_kernel(const uint8_t* frame_hwc, int H, int W, int Hs, int Ws, float scale_y, float scale_x,
                                                         int pad, float* in8, int fill_random, unsigned seed, unsigned index)
{
    __shared__ float byte01[256];      // image.load: byte / 255, a correctly rounded division -- the 256 quotients once per block
    byte01[threadIdx.x] = (float)threadIdx.x / 255.f;
    __syncthreads();
    const int Wp = Ws + 2 * pad;
    const int yp = blockIdx.y, xp = blockIdx.x * 256 + threadIdx.x;
    if (xp >= Wp) return;
    const int y = reflect(yp - pad, Hs), x = reflect(xp - pad, Ws);
    const AxisTap ty = axis_tap(y, H, Hs, scale_y), tx = axis_tap(x, W, Ws, scale_x);
    float rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        rgb[c] = resample(ty, H, [&](int r) {
            const uint8_t* row = frame_hwc + (size_t)r * W * 3 + c;
            return resample(tx, W, [&](int k) { return byte01[row[(size_t)k * 3]]; });
        });
    float4 lo, hi;
    lo.x = rgb[2] * 255.f - 103.939f;      // preprocess.lua:57-62 (BGR, mean-subtracted)
    lo.y = rgb[1] * 255.f - 116.779f;
    lo.z = rgb[0] * 255.f - 123.68f;
    lo.w = 0.f; hi.x = 0.f; hi.y = 0.f;
    if (fill_random) {                     // generate_fill (core.lua:108-117) under a zero certainty, keyed by the SCALED grid's (y, x)
        lo.w = fill_uniform(seed, index, 2, y, x) * 255.f - 103.939f;
        hi.x = fill_uniform(seed, index, 1, y, x) * 255.f - 116.779f;
        hi.y = fill_uniform(seed, index, 0, y, x) * 255.f - 123.68f;
    }
    hi.z = 0.f; hi.w = 0.f;
    float4* o = reinterpret_cast<float4*>(in8 + ((size_t)yp * Wp + xp) * 8);
    o[0] = lo; o[1] = hi;
}

// scale_planar: [C][Hs][Ws] -> [C][Hd][Wd] fp32.  A lane forms VEC consecutive destination samples of one row (VEC == 4: one 16-byte
// store; the launch picks it when the rows of dst are 16-byte aligned)
template <int VEC>
__global__ __launch_bounds__(256) void scale_planar_kernel(const float* src, float* dst, int Hs, int Ws, int Hd, int Wd, float scale_y, float scale_x)
{
    const int y = blockIdx.y, x0 = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (x0 >= Wd) return;
    const float* plane = src + (size_t)blockIdx.z * Hs * Ws;
    const AxisTap ty = axis_tap(y, Hs, Hd, scale_y);
    float v[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const AxisTap tx = axis_tap(x0 + j, Ws, Wd, scale_x);
        v[j] = resample(ty, Hs, [&](int r) {
            const float* row = plane + (size_t)r * Ws;
            return resample(tx, Ws, [&](int k) { return row[k]; });
        });
    }
    float* o = dst + ((size_t)blockIdx.z * Hd + y) * Wd + x0;
    if (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    else o[0] = v[0];
}

inline float axis_scale(int src_len, int dst_len) { return dst_len > 1 ? (float)(src_len - 1) / (float)(dst_len - 1) : 0.f; }

}  // namespace

int launch_scale_prep(const uint8_t* frame_hwc, int H, int W, int Hs, int Ws, int pad, float* in8, hipStream_t st,
                      int fill_random, unsigned seed, unsigned index)
{
    FAV_REQUIRE(H > 0 && W > 0 && Hs > pad && Ws > pad && pad >= 0 && Hs + 2 * pad <= 65535, "scale_prep: bad size %dx%d -> %dx%d (padding %d)", W, H, Ws, Hs, pad);
    hipLaunchKernelGGL(scale_prep_kernel, dim3((Ws + 2 * pad + 255) / 256, Hs + 2 * pad), dim3(256), 0, st, frame_hwc, H, W, Hs, Ws,
                       axis_scale(H, Hs), axis_scale(W, Ws), pad, in8, fill_random, seed, index);
    FAV_LAUNCH_CHECK("scale_prep_kernel");
    return FAV_OK;
}

int launch_scale_planar(const float* src, float* dst, int C, int Hs, int Ws, int Hd, int Wd, hipStream_t st)
{
    FAV_REQUIRE(C > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && C <= 65535 && Hd <= 65535, "scale_planar: bad size [%d] %dx%d -> %dx%d", C, Ws, Hs, Wd, Hd);
    const float sy = axis_scale(Hs, Hd), sx = axis_scale(Ws, Wd);
    if (Wd % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0)
        hipLaunchKernelGGL(scale_planar_kernel<4>, dim3((Wd / 4 + 255) / 256, Hd, C), dim3(256), 0, st, src, dst, Hs, Ws, Hd, Wd, sy, sx);
    else
        hipLaunchKernelGGL(scale_planar_kernel<1>, dim3((Wd + 255) / 256, Hd, C), dim3(256), 0, st, src, dst, Hs, Ws, Hd, Wd, sy, sx);
    FAV_LAUNCH_CHECK("scale_planar_kernel");
    return FAV_OK;
}

}  // namespace fav
