// frame_taps.h -- the bilinear taps of the optical-flow warp (A2: stnbdhw/BilinearSamplerBDHW.cu:48-109, utils.lua:141-149) and the
// reflection of nn.SpatialReflectionPadding, shared by the gather kernels of kernels_frame.hip and kernels_longterm.hip.  Both units are
// compiled with -ffp-contract=off: the fp32 expressions round like the CPU restatement.
#pragma once
#include "fav_internal.h"

namespace fav {

__device__ __forceinline__ int reflect(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// bilinear weights/taps shared by all channels of one output pixel
struct Taps {
    int o00, o01, o10, o11;     // linear offsets y*W+x (clamped so they are always addressable)
    float w00, w01, w10, w11;   // the weights as the reference forms them (NOT zeroed for taps outside the image)
    unsigned in;                // bit k set: tap k lies inside the image; otherwise its VALUE is 0 (BilinearSamplerBDHW.cu:86-101)
};

// FAV_BORDER_STN: BilinearSamplerBDHW.cu:13-23,72-73,92-106.  yf = dy + y, xf = dx + x.
// Bit-exact with the reference kernel compiled for gfx950 (oracle/_ref/libwarp_ref_nofma.so, tests/golden/warp_*.npz): the
// same float -> int conversion (saturating, NaN -> 0), the weights left as computed and the out-of-image VALUES zeroed, so
// that a non-finite weight meets a zero exactly as in the reference (inf x 0 = NaN for infinite flows).
__device__ __forceinline__ Taps taps_stn(float yf, float xf, int H, int W)
{
    Taps t;
    const int x0 = (int)floorf(xf), y0 = (int)floorf(yf);
    const float wx = 1.f - (xf - (float)x0), wy = 1.f - (yf - (float)y0);
    const int x1 = (int)((unsigned)x0 + 1u), y1 = (int)((unsigned)y0 + 1u);          // INT_MAX + 1 wraps like the hardware add
    const bool xi0 = x0 >= 0 && x0 <= W - 1, xi1 = x1 >= 0 && x1 <= W - 1;
    const bool yi0 = y0 >= 0 && y0 <= H - 1, yi1 = y1 >= 0 && y1 <= H - 1;
    const int xc0 = min(max(x0, 0), W - 1), xc1 = min(max(x1, 0), W - 1);
    const int yc0 = min(max(y0, 0), H - 1), yc1 = min(max(y1, 0), H - 1);
    t.o00 = yc0 * W + xc0; t.o01 = yc0 * W + xc1; t.o10 = yc1 * W + xc0; t.o11 = yc1 * W + xc1;
    t.w00 = wx * wy;
    t.w01 = (1.f - wx) * wy;
    t.w10 = wx * (1.f - wy);
    t.w11 = (1.f - wx) * (1.f - wy);
    t.in = (unsigned)(xi0 && yi0) | ((unsigned)(xi1 && yi0) << 1) | ((unsigned)(xi0 && yi1) << 2) | ((unsigned)(xi1 && yi1) << 3);
    return t;
}

// FAV_BORDER_CPU: image.warp(..., 'bilinear', true, 'pad', 0) [Torch7 `image`, recalled]
__device__ __forceinline__ Taps taps_cpu(float iy, float ix, int H, int W)
{
    Taps t;
    if (iy < 0.f || iy > (float)(H - 1) || ix < 0.f || ix > (float)(W - 1)) {
        t.o00 = t.o01 = t.o10 = t.o11 = 0;
        t.w00 = t.w01 = t.w10 = t.w11 = 0.f;
        t.in = 0u;
        return t;
    }
    const int xw = (int)floorf(ix), yn = (int)floorf(iy);
    const int xe = xw + 1, ys = yn + 1;
    t.w00 = ((float)xe - ix) * ((float)ys - iy);
    t.w01 = (ix - (float)xw) * ((float)ys - iy);
    t.w10 = ((float)xe - ix) * (iy - (float)yn);
    t.w11 = (ix - (float)xw) * (iy - (float)yn);
    const int xec = min(xe, W - 1), ysc = min(ys, H - 1);
    t.o00 = yn * W + xw; t.o01 = yn * W + xec; t.o10 = ysc * W + xw; t.o11 = ysc * W + xec;
    t.in = 15u;
    return t;
}

__device__ __forceinline__ Taps make_taps(int border, float yf, float xf, int H, int W)
{
    return border == FAV_BORDER_CPU ? taps_cpu(yf, xf, H, W) : taps_stn(yf, xf, H, W);
}

__device__ __forceinline__ float sample(const float* plane, const Taps& t)
{
    // summation order of BilinearSamplerBDHW.cu:103-106; taps outside the image contribute weight x 0 (:86-101)
    const float v00 = (t.in & 1u) ? plane[t.o00] : 0.f, v01 = (t.in & 2u) ? plane[t.o01] : 0.f;
    const float v10 = (t.in & 4u) ? plane[t.o10] : 0.f, v11 = (t.in & 8u) ? plane[t.o11] : 0.f;
    return t.w00 * v00 + t.w01 * v01 + t.w10 * v10 + t.w11 * v11;
}

// the same four values with the two taps of a row fetched as ONE 8-byte load when they are neighbours in memory (everywhere but at a
// clamped border): half the gather instructions of the fused input assembly, whose three planes share the taps (round 6)
__device__ __forceinline__ float sample_pairs(const float* plane, const Taps& t)
{
    typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
    float v00, v01, v10, v11;
    if (t.o01 == t.o00 + 1) { const f2u a = *reinterpret_cast<const f2u*>(plane + t.o00); v00 = a.x; v01 = a.y; }
    else { v00 = plane[t.o00]; v01 = plane[t.o01]; }
    if (t.o11 == t.o10 + 1) { const f2u b = *reinterpret_cast<const f2u*>(plane + t.o10); v10 = b.x; v11 = b.y; }
    else { v10 = plane[t.o10]; v11 = plane[t.o11]; }
    v00 = (t.in & 1u) ? v00 : 0.f; v01 = (t.in & 2u) ? v01 : 0.f; v10 = (t.in & 4u) ? v10 : 0.f; v11 = (t.in & 8u) ? v11 : 0.f;
    return t.w00 * v00 + t.w01 * v01 + t.w10 * v10 + t.w11 * v11;
}

}  // namespace fav
