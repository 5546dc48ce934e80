// kernels_equi.hip -- the transform stage of the 360-degree pipeline for gfx950: one equirectangular frame -> the six expanded cube
// faces fav_vr_* works on (what transformVRVideo.sh has an ffmpeg with the transform360 filter write, cube_edge_length=768,
// expand_coef=1.2).  The geometry is the INVERSE of the project's own cube -> equirectangular map (vr.cpp, equirect_map:
// vr_helper.lua:95-184 on the strip of fast_artistic_video_vr.lua:543), not transform360's source; the filter is Catmull-Rom on a
// regular sub-pixel grid, not transform360's Lanczos-4 + low-pass (quality against it: unmeasured).
//
// Face k is processing position k (strip segment k; segments 4 and 5 enter the strip rotated by 180 degrees).  A point (fx, fy) of
// face k, in pixel indices:
//   (sx, sy) = k < 4 ? (fx, fy) : (wplus - 1 - fx, hplus - 1 - fy)                          the strip's orientation
//   a = (sx - overlap_w / 2) * (2 / (wplus - overlap_w)) - 1,  b likewise along y          -1 .. 1 on the inner face, beyond it on the margin
//   (x, y, z) = k: 0 (a, b, 1)   1 (-1, b, a)   2 (1, b, -a)   3 (-a, b, -1)   4 (a, -1, b)   5 (a, 1, -b)
//   phi = atan2(-x, -z) (+ 2 pi when negative),  theta = atan2(sqrt(x^2 + z^2), y)
//   (u, v) = (phi * W / (2 pi), H - theta * H / pi)                                        pixel index i <-> phi = 2 pi i / W, row j <-> theta = pi (1 - j / H)
// and the equirectangular image is sampled at (u, v): the cubic of cubic.h along the row through columns floor(u) - 1 .. + 2 (modulo W),
// then along the column through rows floor(v) - 1 .. + 2 (clamped to 0 .. H - 1).  An output pixel is the mean of S x S such samples at
// (fx + (2 i + 1 - S) / (2 S), fy + (2 j + 1 - S) / (2 S)), summed row by row.  All of it in fp32, every operation rounded as written
// (-ffp-contract=off); tests/util/equi_model.py restates it.
//
// One launch, the face in blockIdx.z, one output pixel per lane, 64 x 4 pixels per block; the six (+ six) output pointers travel by value
// in the kernel arguments.  A gather: 48 u8 taps per sub-sample, neighbouring lanes a fraction of a source pixel apart, so the vector L1
// and the L2 serve them and the source leaves HBM about once; 3 bytes (+ 12 with the fp32 plane) are stored per pixel.
#include "cubic.h"
#include "fav_internal.h"

namespace fav {
namespace {

struct EquiFaces { uint8_t* u8[6]; float* f32[6]; };

struct EquiGeom {
    int ew, eh, hplus, wplus, S;
    float half_ov_w, half_ov_h;      // overlap / 2
    float ka, kb;                    // 2 / (wplus - overlap_w), 2 / (hplus - overlap_h)
    float cu, cv;                    // W / (2 pi), H / pi
};

__global__ __launch_bounds__(256) void equi_to_faces_kernel(const uint8_t* __restrict__ equi, EquiGeom g, EquiFaces out)
{
    const int fx = blockIdx.x * 64 + threadIdx.x, fy = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (fx >= g.wplus || fy >= g.hplus) return;
    const float two_s = (float)(2 * g.S);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < g.S; ++j) {
        const float py = (float)fy + (float)(2 * j + 1 - g.S) / two_s;
        const float sy = k < 4 ? py : (float)(g.hplus - 1) - py;
        const float b = (sy - g.half_ov_h) * g.kb - 1.f;
        for (int i = 0; i < g.S; ++i) {
            const float px = (float)fx + (float)(2 * i + 1 - g.S) / two_s;
            const float sx = k < 4 ? px : (float)(g.wplus - 1) - px;
            const float a = (sx - g.half_ov_w) * g.ka - 1.f;
            float x, y, z;
            switch (k) {
            case 0:  x = a;    y = b;    z = 1.f;  break;
            case 1:  x = -1.f; y = b;    z = a;    break;
            case 2:  x = 1.f;  y = b;    z = -a;   break;
            case 3:  x = -a;   y = b;    z = -1.f; break;
            case 4:  x = a;    y = -1.f; z = b;    break;
            default: x = a;    y = 1.f;  z = -b;   break;
            }
            float phi = atan2f(-x, -z);
            if (phi < 0.f) phi = phi + 6.2831853071795864769f;
            const float theta = atan2f(sqrtf(x * x + z * z), y);
            const float u = phi * g.cu, v = (float)g.eh - theta * g.cv;
            const float fu = floorf(u), fv = floorf(v);
            const float tx = u - fu, ty = v - fv;
            const int iu = (int)fu, iv = (int)fv;
            int col[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) col[t] = ((iu + g.ew - 1 + t) % g.ew) * 3;      // iu in 0 .. ew: never negative
            float rows[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = min(max(iv - 1 + r, 0), g.eh - 1);
                const uint8_t* p = equi + (size_t)row * g.ew * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    rows[r][c] = catmull_rom((float)p[col[0] + c], (float)p[col[1] + c], (float)p[col[2] + c], (float)p[col[3] + c], tx);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + catmull_rom(rows[0][c], rows[1][c], rows[2][c], rows[3][c], ty);
        }
    }
    const float n = (float)(g.S * g.S);
    const size_t o = ((size_t)fy * g.wplus + fx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float m = acc[c] / n;
        out.u8[k][o + c] = (uint8_t)fminf(fmaxf(floorf(m + 0.5f), 0.f), 255.f);
        if (out.f32[k]) out.f32[k][o + c] = m;
    }
}

}  // namespace

int launch_equi_to_faces(const uint8_t* equi_rgb_hwc, int ew, int eh, int hplus, int wplus, int overlap_w, int overlap_h, int supersample,
                         uint8_t* const* faces_u8, float* const* faces_f32_or_null, hipStream_t st)
{
    EquiGeom g;
    g.ew = ew; g.eh = eh; g.hplus = hplus; g.wplus = wplus; g.S = supersample;
    g.half_ov_w = (float)overlap_w * 0.5f; g.half_ov_h = (float)overlap_h * 0.5f;
    g.ka = 2.f / (float)(wplus - overlap_w); g.kb = 2.f / (float)(hplus - overlap_h);
    g.cu = (float)((double)ew / 6.28318530717958647692); g.cv = (float)((double)eh / 3.14159265358979323846);
    EquiFaces out;
    for (int k = 0; k < 6; ++k) { out.u8[k] = faces_u8[k]; out.f32[k] = faces_f32_or_null ? faces_f32_or_null[k] : nullptr; }
    hipLaunchKernelGGL(equi_to_faces_kernel, dim3((wplus + 63) / 64, (hplus + 3) / 4, 6), dim3(64, 4), 0, st, equi_rgb_hwc, g, out);
    FAV_LAUNCH_CHECK("equi_to_faces_kernel");
    return FAV_OK;
}

}  // namespace fav
