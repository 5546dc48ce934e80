// tconv_pack.h -- phase / tap tables and host-side weight packing of a transposed convolution (nn.SpatialFullConvolution: `u<n>` and
// `f<k>s<s>-<n>`, models_video.lua:81-89,99-102; kernels_tconv.hip).  Plain C++ (no HIP): the CPU test suite compiles it on its own.
//
//     out[co][oy][ox] = b[co] + sum_ci sum_ky sum_kx x[ci][iy][ix] * w[ci][co][ky][kx],   oy = iy * s - p + ky,  ox = ix * s - p + kx
//
// Along one axis, write o = s * u + c (c = o mod s: the output PHASE, u = o div s).  Then o + p = s * (u + d) + r with
// r = (c + p) mod s, d = (c + p) div s, and only the taps ky = r + s * j (j = 0 .. ceil((k - r) / s) - 1) reach o, from the input
// i = (o + p - ky) / s = u + d - j.  So phase c is a stride-1 correlation over the PHYSICAL input with ntap(c) taps:
//     tap j of phase c:  kernel index  r + s * j,   input offset  d - j  (relative to u)
// and the s * s two-dimensional phases (cy, cx) share the k * k taps of the filter: k^2 / s^2 multiplies per output instead of the k^2
// that the zero-stuffed form spends.  The offsets of all phases lie in [lo, hi] (lo <= 0 <= hi for p <= k - 1): the halo of a tile.
//
// Tap SLOTS: the k * k taps in the order the kernel consumes them -- phase (cy, cx) major (cy * s + cx), then (jy, jx) row-major.
// Packed order (what one wave streams: it owns one phase and one tile of 32 output channels):
//     out[tconv_pack_index(...)] = out[(((nt * (cinp / 8) + kg) * k * k + slot) * 64 + lane) * 4 + st]
//     nt = tile of 32 output channels (a GROUP: block nt is the packing of filters 32 nt .. 32 nt + 31 alone), kg = group of 8 input
//     channels, lane = h * 32 + n (output channel nt * 32 + n), MFMA step st multiplies input channels kg * 8 + st (h = 0) and
//     kg * 8 + 4 + st (h = 1).  Input channels >= cin and output channels >= cout are zero.
#pragma once
#include <cstddef>
#include <vector>

#ifdef __HIPCC__
#define FAV_TCONV_HD __host__ __device__
#else
#define FAV_TCONV_HD
#endif

namespace fav {

constexpr int TCONV_MAX_K = 9, TCONV_MAX_S = 4;
constexpr int TCONV_TILE_H = 8, TCONV_TILE_W = 32;      // the kernel's tile, in u coordinates (input pixels): 8 s x 32 s output pixels

// one axis, phase c = o mod s
FAV_TCONV_HD inline int tconv_ntap(int k, int s, int p, int c) { const int r = (c + p) % s; return r < k ? (k - r + s - 1) / s : 0; }
FAV_TCONV_HD inline int tconv_tap_k(int s, int p, int c, int j) { return (c + p) % s + s * j; }       // kernel index of tap j
FAV_TCONV_HD inline int tconv_tap_off(int s, int p, int c, int j) { return (c + p) / s - j; }          // input index - u
// smallest / largest input offset over all phases (the halo: -lo rows above / left, hi below / right)
FAV_TCONV_HD inline int tconv_lo(int k, int s, int p)
{
    int lo = 0;
    for (int c = 0; c < s; ++c) { const int n = tconv_ntap(k, s, p, c); if (n > 0 && tconv_tap_off(s, p, c, n - 1) < lo) lo = tconv_tap_off(s, p, c, n - 1); }
    return lo;
}
FAV_TCONV_HD inline int tconv_hi(int k, int s, int p)
{
    int hi = 0;
    for (int c = 0; c < s; ++c) if (tconv_ntap(k, s, p, c) > 0 && tconv_tap_off(s, p, c, 0) > hi) hi = tconv_tap_off(s, p, c, 0);
    return hi;
}
// first tap slot of the two-dimensional phase (cy, cx); the taps of one axis sum to k over its phases
FAV_TCONV_HD inline int tconv_slot0(int k, int s, int p, int cy, int cx)
{
    int n = 0;
    for (int c = 0; c < cy; ++c) n += tconv_ntap(k, s, p, c) * k;
    for (int c = 0; c < cx; ++c) n += tconv_ntap(k, s, p, cy) * tconv_ntap(k, s, p, c);
    return n;
}
FAV_TCONV_HD inline int tconv_slot(int k, int s, int p, int cy, int cx, int jy, int jx)
{
    return tconv_slot0(k, s, p, cy, cx) + jy * tconv_ntap(k, s, p, cx) + jx;
}

inline size_t tconv_packed_floats(int cinp, int coutp, int k) { return (size_t)(coutp / 32) * (cinp / 8) * k * k * 256; }
// where the weight of (output channel co, input channel ci, tap slot) sits
FAV_TCONV_HD inline size_t tconv_pack_index(int cinp, int k, int co, int ci, int slot)
{
    return ((((size_t)(co >> 5) * (cinp >> 3) + (ci >> 3)) * k * k + slot) * 64 + ((ci >> 2) & 1) * 32 + (co & 31)) * 4 + (ci & 3);
}

// w: [cin][cout][k][k] (nn.SpatialFullConvolution), cin <= cinp (a multiple of 8), cout <= coutp (a multiple of 32)
inline void conv_tconv_pack(const float* w, int cin, int cout, int cinp, int coutp, int k, int s, int p, std::vector<float>& out)
{
    out.assign(tconv_packed_floats(cinp, coutp, k), 0.f);
    for (int cy = 0; cy < s; ++cy)
        for (int cx = 0; cx < s; ++cx)
            for (int jy = 0; jy < tconv_ntap(k, s, p, cy); ++jy)
                for (int jx = 0; jx < tconv_ntap(k, s, p, cx); ++jx) {
                    const int slot = tconv_slot(k, s, p, cy, cx, jy, jx), ky = tconv_tap_k(s, p, cy, jy), kx = tconv_tap_k(s, p, cx, jx);
                    for (int ci = 0; ci < cin; ++ci)
                        for (int co = 0; co < cout; ++co)
                            out[tconv_pack_index(cinp, k, co, ci, slot)] = w[(((size_t)ci * cout + co) * k + ky) * k + kx];
                }
}

// the same layer as the ordinary convolution it is at stride 1: [cin][cout][k][k] -> [cout][cin][k][k] with both axes flipped (zero padding k - 1 - p)
inline void conv_tconv_as_conv(const float* w, int cin, int cout, int k, std::vector<float>& out)
{
    out.resize((size_t)cin * cout * k * k);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx)
                    out[(((size_t)co * cin + ci) * k + ky) * k + kx] = w[(((size_t)ci * cout + co) * k + (k - 1 - ky)) * k + (k - 1 - kx)];
}

}  // namespace fav
