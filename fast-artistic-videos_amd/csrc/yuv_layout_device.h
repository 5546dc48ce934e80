// yuv_layout_device.h -- the lane's 2 x 8 block of kernels_yuv_layout.hip: the block of yuv_device.h once more, on a SAMPLE TYPE (one byte,
// or two bytes little-endian for 9 .. 16 bits) and with 4:2:2 next to 4:2:0 and 4:4:4.  The depth is in the constants (YuvLK: the chroma
// offset 2^(D-1) and the largest sample 2^D - 1 join those of YuvK), never a branch.  yuv_device.h is included for what does not depend
// on the sample -- the unaligned vector types, the byte rules, the sources, the block's position -- and is not changed: the 8-bit 4:2:0 /
// 4:4:4 kernels compile to what they compiled to.  Every unit that includes this is compiled with -ffp-contract=off.
#pragma once
#include "yuv_device.h"

namespace fav {

struct YuvLK { float kr, kg, kb, sy, oy, cbs, crs, isy, kR, kB, kGr, kGb, oc, qmax; };

// include/fav_yuv.h: m = 2^(D-8), q = (2^D - 1)/255; every constant in double, rounded once.  At D = 8 these are yuv_constants'.
inline YuvLK yuv_layout_constants(const fav_yuv_layout& l)
{
    const double kr = l.matrix == FAV_YUV_BT709 ? 0.2126 : 0.299, kb = l.matrix == FAV_YUV_BT709 ? 0.0722 : 0.114;
    const double kg = 1.0 - kr - kb;
    const double m = (double)(1u << (l.depth - 8)), q = (double)((1u << l.depth) - 1u) / 255.0;
    const double sy = l.full_range ? q : 219.0 / 255.0 * m, sc = l.full_range ? q : 224.0 / 255.0 * m, oy = l.full_range ? 0.0 : 16.0 * m;
    const double k_r = 2.0 * (1.0 - kr) / sc, k_b = 2.0 * (1.0 - kb) / sc;
    YuvLK k;
    k.kr = (float)kr; k.kg = (float)kg; k.kb = (float)kb; k.sy = (float)sy; k.oy = (float)oy;
    k.cbs = (float)(sc / (2.0 * (1.0 - kb))); k.crs = (float)(sc / (2.0 * (1.0 - kr)));
    k.isy = (float)(1.0 / sy); k.kR = (float)k_r; k.kB = (float)k_b; k.kGr = (float)(k_r * kr / kg); k.kGb = (float)(k_b * kb / kg);
    k.oc = (float)(1u << (l.depth - 1)); k.qmax = (float)((1u << l.depth) - 1u);
    return k;
}

// the first three are yuv_device.h's modes
enum { YL_420_CENTER = YUV_420_CENTER, YL_420_LEFT = YUV_420_LEFT, YL_444 = YUV_444, YL_422_CENTER = 3, YL_422_LEFT = 4 };
inline int yuv_layout_mode(const fav_yuv_layout& l)
{
    if (l.chroma == FAV_YUV_444) return YL_444;
    const bool left = l.siting == FAV_YUV_SITING_LEFT;
    return l.chroma == FAV_YUV_422 ? (left ? YL_422_LEFT : YL_422_CENTER) : (left ? YL_420_LEFT : YL_420_CENTER);
}
constexpr bool yl_is_420(int mode) { return mode == YL_420_CENTER || mode == YL_420_LEFT; }
constexpr bool yl_is_422(int mode) { return mode == YL_422_CENTER || mode == YL_422_LEFT; }
constexpr bool yl_is_left(int mode) { return mode == YL_420_LEFT || mode == YL_422_LEFT; }

struct __attribute__((packed, aligned(1))) B16 { uint32_t v[4]; };       // a row of 8 two-byte samples at any byte address
struct __attribute__((packed, aligned(1))) U16 { uint16_t v; };          // one two-byte sample at any byte address

// A plane is addressed in bytes (a 16-bit plane may start at an odd address); idx counts samples.  row8 / row4: the 8 luma (4 chroma)
// samples of a full block's row in one access.
template <class T> struct Smp;
template <> struct Smp<uint8_t> {
    static constexpr int BYTES = 1;
    static __device__ __forceinline__ float ld(const uint8_t* p, size_t idx) { return (float)p[idx]; }
    static __device__ __forceinline__ void st(uint8_t* p, size_t idx, uint32_t q) { p[idx] = (uint8_t)q; }
    static __device__ __forceinline__ void ld_row8(const uint8_t* p, size_t idx, float* o)
    {
        const B8 v = *reinterpret_cast<const B8*>(p + idx);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = byte_of(v.v, i);
    }
    static __device__ __forceinline__ void ld_row4(const uint8_t* p, size_t idx, float* o)
    {
        const uint32_t v = reinterpret_cast<const B4*>(p + idx)->v;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = byte_of(&v, i);
    }
    static __device__ __forceinline__ void st_row8(uint8_t* p, size_t idx, const uint32_t* q) { store_row8(p + idx, q); }
    static __device__ __forceinline__ void st_row4(uint8_t* p, size_t idx, const uint32_t* q)
    {
        B4 o;
        o.v = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
        *reinterpret_cast<B4*>(p + idx) = o;
    }
};
template <> struct Smp<uint16_t> {
    static constexpr int BYTES = 2;
    static __device__ __forceinline__ float half_of(const uint32_t* w, int i) { return (float)((w[i >> 1] >> (16 * (i & 1))) & 65535u); }
    static __device__ __forceinline__ float ld(const uint8_t* p, size_t idx) { return (float)reinterpret_cast<const U16*>(p + 2 * idx)->v; }
    static __device__ __forceinline__ void st(uint8_t* p, size_t idx, uint32_t q) { U16 o; o.v = (uint16_t)q; *reinterpret_cast<U16*>(p + 2 * idx) = o; }
    static __device__ __forceinline__ void ld_row8(const uint8_t* p, size_t idx, float* o)
    {
        const B16 v = *reinterpret_cast<const B16*>(p + 2 * idx);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = half_of(v.v, i);
    }
    static __device__ __forceinline__ void ld_row4(const uint8_t* p, size_t idx, float* o)
    {
        const B8 v = *reinterpret_cast<const B8*>(p + 2 * idx);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = half_of(v.v, i);
    }
    static __device__ __forceinline__ void st_row8(uint8_t* p, size_t idx, const uint32_t* q)
    {
        B16 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = q[2 * j] | q[2 * j + 1] << 16;
        *reinterpret_cast<B16*>(p + 2 * idx) = o;
    }
    static __device__ __forceinline__ void st_row4(uint8_t* p, size_t idx, const uint32_t* q)
    {
        B8 o;
        o.v[0] = q[0] | q[1] << 16; o.v[1] = q[2] | q[3] << 16;
        *reinterpret_cast<B8*>(p + 2 * idx) = o;
    }
};

__device__ __forceinline__ uint32_t quant_to(float x, float qmax) { return (uint32_t)fminf(fmaxf(floorf(x + 0.5f), 0.f), qmax); }

__device__ __forceinline__ void encode_pixel(const YuvLK& k, float R, float G, float B, float& Y, float& Cb, float& Cr)
{
    const float y = (k.kr * R + k.kg * G) + k.kb * B;
    Y = y * k.sy + k.oy;
    Cb = (B - y) * k.cbs + k.oc;
    Cr = (R - y) * k.crs + k.oc;
}

// the third source: planar fp32 [3][H][W] UNQUANTISED (deep outputs): clamp to [0, 1], x255, no truncation
__device__ __forceinline__ float unit_to_255(float v) { return fminf(fmaxf(v, 0.f), 1.f) * 255.f; }
struct SrcF32Raw {
    const float* rgbf; int W; size_t plane;
    __device__ __forceinline__ void pixel(int x, int y, float& R, float& G, float& B) const
    {
        const size_t p = (size_t)y * W + x;
        R = unit_to_255(rgbf[p]); G = unit_to_255(rgbf[plane + p]); B = unit_to_255(rgbf[2 * plane + p]);
    }
    __device__ __forceinline__ void row8(int x0, int y, float* R, float* G, float* B) const
    {
        const size_t p = (size_t)y * W + x0;
        const F8 fr = *reinterpret_cast<const F8*>(rgbf + p), fg = *reinterpret_cast<const F8*>(rgbf + plane + p),
                 fb = *reinterpret_cast<const F8*>(rgbf + 2 * plane + p);
#pragma unroll
        for (int i = 0; i < YUV_BW; ++i) { R[i] = unit_to_255(fr.v[i]); G[i] = unit_to_255(fg.v[i]); B[i] = unit_to_255(fb.v[i]); }
    }
};

// one lane's block of the source's image -> the frame's planes.  The lane forms its own chroma samples: 1 x 4 (4:2:0), 2 x 4 (4:2:2),
// 2 x 8 (4:4:4).
template <int MODE, class T, class Src>
__device__ __forceinline__ void yuv_layout_encode_block(const Src& src, int W, int H, const YuvLK& k, uint8_t* __restrict__ yuv)
{
    using S = Smp<T>;
    int bx, by;
    if (!yuv_block_of(W, H, bx, by)) return;
    const int x0 = bx * YUV_BW, y0 = by * 2;
    const bool full = x0 + YUV_BW <= W && y0 + 2 <= H;
    const size_t plane = (size_t)W * H;
    const int Wc = MODE == YL_444 ? W : (W + 1) / 2, Hc = yl_is_420(MODE) ? (H + 1) / 2 : H;
    uint8_t* const Yp = yuv;
    uint8_t* const Cbp = yuv + plane * S::BYTES;
    uint8_t* const Crp = Cbp + (size_t)Wc * Hc * S::BYTES;

    uint32_t yq[2][YUV_BW];
    float cb[2][YUV_BW], cr[2][YUV_BW];
    float cbl[2] = {0.f, 0.f}, crl[2] = {0.f, 0.f};       // left siting: the chroma of column x0 - 1 (clamped)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = min(y0 + r, H - 1);
        float R[YUV_BW], G[YUV_BW], B[YUV_BW];
        if (full) src.row8(x0, y, R, G, B);
        else {
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i) src.pixel(min(x0 + i, W - 1), y, R[i], G[i], B[i]);
        }
#pragma unroll
        for (int i = 0; i < YUV_BW; ++i) {
            float Y;
            encode_pixel(k, R[i], G[i], B[i], Y, cb[r][i], cr[r][i]);
            yq[r][i] = quant_to(Y, k.qmax);
        }
        if (yl_is_left(MODE)) {
            float Rl, Gl, Bl, Yl;
            src.pixel(max(x0 - 1, 0), y, Rl, Gl, Bl);
            encode_pixel(k, Rl, Gl, Bl, Yl, cbl[r], crl[r]);
        }
    }

    uint32_t cbq[2][YUV_BW], crq[2][YUV_BW];
    if (MODE == YL_444) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i) { cbq[r][i] = quant_to(cb[r][i], k.qmax); crq[r][i] = quant_to(cr[r][i], k.qmax); }
    } else if (MODE == YL_420_CENTER) {
#pragma unroll
        for (int j = 0; j < YUV_BW / 2; ++j) {
            cbq[0][j] = quant_to(((cb[0][2 * j] + cb[0][2 * j + 1]) + (cb[1][2 * j] + cb[1][2 * j + 1])) * 0.25f, k.qmax);
            crq[0][j] = quant_to(((cr[0][2 * j] + cr[0][2 * j + 1]) + (cr[1][2 * j] + cr[1][2 * j + 1])) * 0.25f, k.qmax);
        }
    } else if (MODE == YL_422_CENTER) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < YUV_BW / 2; ++j) {
                cbq[r][j] = quant_to((cb[r][2 * j] + cb[r][2 * j + 1]) * 0.5f, k.qmax);
                crq[r][j] = quant_to((cr[r][2 * j] + cr[r][2 * j + 1]) * 0.5f, k.qmax);
            }
    } else {      // left siting: 1-2-1 along x at the even column; 4:2:0 then takes the mean of the two rows
#pragma unroll
        for (int j = 0; j < YUV_BW / 2; ++j) {
            float hb[2], hr[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float lb = j ? cb[r][2 * j - 1] : cbl[r], lr = j ? cr[r][2 * j - 1] : crl[r];
                hb[r] = ((lb + cb[r][2 * j + 1]) + (cb[r][2 * j] + cb[r][2 * j])) * 0.25f;
                hr[r] = ((lr + cr[r][2 * j + 1]) + (cr[r][2 * j] + cr[r][2 * j])) * 0.25f;
            }
            if (MODE == YL_420_LEFT) {
                cbq[0][j] = quant_to((hb[0] + hb[1]) * 0.5f, k.qmax);
                crq[0][j] = quant_to((hr[0] + hr[1]) * 0.5f, k.qmax);
            } else {
#pragma unroll
                for (int r = 0; r < 2; ++r) { cbq[r][j] = quant_to(hb[r], k.qmax); crq[r][j] = quant_to(hr[r], k.qmax); }
            }
        }
    }

    if (full) {
#pragma unroll
        for (int r = 0; r < 2; ++r) S::st_row8(Yp, (size_t)(y0 + r) * W + x0, yq[r]);
        if (MODE == YL_444) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                S::st_row8(Cbp, (size_t)(y0 + r) * W + x0, cbq[r]);
                S::st_row8(Crp, (size_t)(y0 + r) * W + x0, crq[r]);
            }
        } else if (yl_is_422(MODE)) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                S::st_row4(Cbp, (size_t)(y0 + r) * Wc + x0 / 2, cbq[r]);
                S::st_row4(Crp, (size_t)(y0 + r) * Wc + x0 / 2, crq[r]);
            }
        } else {
            S::st_row4(Cbp, (size_t)by * Wc + x0 / 2, cbq[0]);
            S::st_row4(Crp, (size_t)by * Wc + x0 / 2, crq[0]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i)
                if (x0 + i < W && y0 + r < H) {
                    const size_t p = (size_t)(y0 + r) * W + x0 + i;
                    S::st(Yp, p, yq[r][i]);
                    if (MODE == YL_444) { S::st(Cbp, p, cbq[r][i]); S::st(Crp, p, crq[r][i]); }
                }
        if (MODE != YL_444) {
#pragma unroll
            for (int r = 0; r < (yl_is_422(MODE) ? 2 : 1); ++r)
#pragma unroll
                for (int j = 0; j < YUV_BW / 2; ++j)
                    if (x0 / 2 + j < Wc && (yl_is_420(MODE) || y0 + r < H)) {
                        const size_t c = (size_t)(yl_is_422(MODE) ? y0 + r : by) * Wc + x0 / 2 + j;
                        S::st(Cbp, c, cbq[r][j]); S::st(Crp, c, crq[r][j]);
                    }
        }
    }
}

}  // namespace fav
