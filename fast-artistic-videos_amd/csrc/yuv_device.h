// yuv_device.h -- what the units that write a frame's YCbCr planes share: the constants, the byte rules, the unaligned vector types and
// the lane's 2 x 8 encode block of kernels_yuv.hip, which says what the arithmetic is and why the block has this shape.  The block
// takes its RGB bytes from a SOURCE: the bytes of an image or the quantised fp32 planes (kernels_yuv.hip), or an image formed in
// registers (kernels_color.hip) -- one definition of the encode and of the 4:2:0 reduction behind all of them.
// Every unit that includes this is compiled with -ffp-contract=off.
#pragma once
#include "fav_internal.h"

namespace fav {

struct YuvK { float kr, kg, kb, sy, oy, cbs, crs, isy, kR, kB, kGr, kGb; };

inline YuvK yuv_constants(const fav_yuv_format& f)
{
    const double kr = f.matrix == FAV_YUV_BT709 ? 0.2126 : 0.299, kb = f.matrix == FAV_YUV_BT709 ? 0.0722 : 0.114;
    const double kg = 1.0 - kr - kb;
    const double sy = f.full_range ? 1.0 : 219.0 / 255.0, sc = f.full_range ? 1.0 : 224.0 / 255.0, oy = f.full_range ? 0.0 : 16.0;
    const double k_r = 2.0 * (1.0 - kr) / sc, k_b = 2.0 * (1.0 - kb) / sc;
    YuvK k;
    k.kr = (float)kr; k.kg = (float)kg; k.kb = (float)kb; k.sy = (float)sy; k.oy = (float)oy;
    k.cbs = (float)(sc / (2.0 * (1.0 - kb))); k.crs = (float)(sc / (2.0 * (1.0 - kr)));
    k.isy = (float)(1.0 / sy); k.kR = (float)k_r; k.kB = (float)k_b; k.kGr = (float)(k_r * kr / kg); k.kGb = (float)(k_b * kb / kg);
    return k;
}

enum { YUV_420_CENTER = 0, YUV_420_LEFT = 1, YUV_444 = 2 };
constexpr int YUV_BW = 8;       // columns of a lane's block (2 rows)
constexpr int YUV_NT = 256;

inline int yuv_mode(const fav_yuv_format& f) { return f.chroma == FAV_YUV_444 ? YUV_444 : f.siting == FAV_YUV_SITING_LEFT ? YUV_420_LEFT : YUV_420_CENTER; }
inline unsigned yuv_grid(int W, int H) { return (unsigned)((((long long)(W + YUV_BW - 1) / YUV_BW) * ((H + 1) / 2) + YUV_NT - 1) / YUV_NT); }

// vector accesses at any byte address (fp32 planes: any dword address)
struct __attribute__((packed, aligned(1))) B4 { uint32_t v; };
struct __attribute__((packed, aligned(1))) B8 { uint32_t v[2]; };
struct __attribute__((packed, aligned(1))) B24 { uint32_t v[6]; };
struct __attribute__((packed, aligned(4))) F8 { float v[8]; };

__device__ __forceinline__ float byte_of(const uint32_t* w, int i) { return (float)((w[i >> 2] >> (8 * (i & 3))) & 255u); }
__device__ __forceinline__ float quantf(float x) { return fminf(fmaxf(floorf(x + 0.5f), 0.f), 255.f); }
__device__ __forceinline__ uint32_t quant(float x) { return (uint32_t)quantf(x); }
// image.save (quantize_kernel, fav_png_encode_f32): clamp to [0, 1], x255, truncate
__device__ __forceinline__ float save_byte(float v) { return (float)(int)(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

__device__ __forceinline__ void encode_pixel(const YuvK& k, float R, float G, float B, float& Y, float& Cb, float& Cr)
{
    const float y = (k.kr * R + k.kg * G) + k.kb * B;
    Y = y * k.sy + k.oy;
    Cb = (B - y) * k.cbs + 128.f;
    Cr = (R - y) * k.crs + 128.f;
}

__device__ __forceinline__ void store_row8(uint8_t* dst, const uint32_t* q)      // 8 samples -> one 8-byte store
{
    B8 o;
    o.v[0] = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
    o.v[1] = q[4] | q[5] << 8 | q[6] << 16 | q[7] << 24;
    *reinterpret_cast<B8*>(dst) = o;
}

// The sources of an encode: pixel() gives one pixel, row8() the 8 pixels of a block's row that lies inside the image (vector loads);
// the values are bytes held as floats, coordinates are inside the image.
struct SrcRgb8 {            // [H][W][3] u8
    const uint8_t* rgb; int W;
    __device__ __forceinline__ void pixel(int x, int y, float& R, float& G, float& B) const
    {
        const size_t p = (size_t)y * W + x;
        R = (float)rgb[3 * p]; G = (float)rgb[3 * p + 1]; B = (float)rgb[3 * p + 2];
    }
    __device__ __forceinline__ void row8(int x0, int y, float* R, float* G, float* B) const
    {
        const B24 px = *reinterpret_cast<const B24*>(rgb + 3 * ((size_t)y * W + x0));
#pragma unroll
        for (int i = 0; i < YUV_BW; ++i) { R[i] = byte_of(px.v, 3 * i); G[i] = byte_of(px.v, 3 * i + 1); B[i] = byte_of(px.v, 3 * i + 2); }
    }
};
struct SrcF32 {             // planar fp32 [3][H][W], image.save's quantisation in front
    const float* rgbf; int W; size_t plane;
    __device__ __forceinline__ void pixel(int x, int y, float& R, float& G, float& B) const
    {
        const size_t p = (size_t)y * W + x;
        R = save_byte(rgbf[p]); G = save_byte(rgbf[plane + p]); B = save_byte(rgbf[2 * plane + p]);
    }
    __device__ __forceinline__ void row8(int x0, int y, float* R, float* G, float* B) const
    {
        const size_t p = (size_t)y * W + x0;
        const F8 fr = *reinterpret_cast<const F8*>(rgbf + p), fg = *reinterpret_cast<const F8*>(rgbf + plane + p),
                 fb = *reinterpret_cast<const F8*>(rgbf + 2 * plane + p);
#pragma unroll
        for (int i = 0; i < YUV_BW; ++i) { R[i] = save_byte(fr.v[i]); G[i] = save_byte(fg.v[i]); B[i] = save_byte(fb.v[i]); }
    }
};

// the block's position: lane idx of the launch owns rows y0, y0 + 1 and columns x0 .. x0 + 7; false: the lane is beyond the frame
__device__ __forceinline__ bool yuv_block_of(int W, int H, int& bx, int& by)
{
    const int nbx = (W + YUV_BW - 1) / YUV_BW, nby = (H + 1) / 2;
    const unsigned idx = blockIdx.x * YUV_NT + threadIdx.x;       // (W * H <= 2^28: the blocks of a frame number below 2^28)
    if (idx >= (unsigned)nbx * (unsigned)nby) return false;
    by = (int)(idx / (unsigned)nbx); bx = (int)(idx - (unsigned)by * (unsigned)nbx);
    return true;
}

// one lane's block of the source's image -> the frame's planes
template <int MODE, class Src>
__device__ __forceinline__ void yuv_encode_block(const Src& src, int W, int H, const YuvK& k, uint8_t* __restrict__ yuv)
{
    int bx, by;
    if (!yuv_block_of(W, H, bx, by)) return;
    const int x0 = bx * YUV_BW, y0 = by * 2;
    const bool full = x0 + YUV_BW <= W && y0 + 2 <= H;
    const size_t plane = (size_t)W * H;
    const int Wc = MODE == YUV_444 ? W : (W + 1) / 2, Hc = MODE == YUV_444 ? H : (H + 1) / 2;
    uint8_t* const Yp = yuv;
    uint8_t* const Cbp = yuv + plane;
    uint8_t* const Crp = Cbp + (size_t)Wc * Hc;

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
            yq[r][i] = quant(Y);
        }
        if (MODE == YUV_420_LEFT) {
            float Rl, Gl, Bl, Yl;
            src.pixel(max(x0 - 1, 0), y, Rl, Gl, Bl);
            encode_pixel(k, Rl, Gl, Bl, Yl, cbl[r], crl[r]);
        }
    }

    // the lane's chroma samples: 2 x 8 (4:4:4) or 1 x 4 (4:2:0)
    uint32_t cbq[2][YUV_BW], crq[2][YUV_BW];
    if (MODE == YUV_444) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i) { cbq[r][i] = quant(cb[r][i]); crq[r][i] = quant(cr[r][i]); }
    } else if (MODE == YUV_420_CENTER) {
#pragma unroll
        for (int j = 0; j < YUV_BW / 2; ++j) {
            cbq[0][j] = quant(((cb[0][2 * j] + cb[0][2 * j + 1]) + (cb[1][2 * j] + cb[1][2 * j + 1])) * 0.25f);
            crq[0][j] = quant(((cr[0][2 * j] + cr[0][2 * j + 1]) + (cr[1][2 * j] + cr[1][2 * j + 1])) * 0.25f);
        }
    } else {
#pragma unroll
        for (int j = 0; j < YUV_BW / 2; ++j) {
            float hb[2], hr[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float lb = j ? cb[r][2 * j - 1] : cbl[r], lr = j ? cr[r][2 * j - 1] : crl[r];
                hb[r] = ((lb + cb[r][2 * j + 1]) + (cb[r][2 * j] + cb[r][2 * j])) * 0.25f;
                hr[r] = ((lr + cr[r][2 * j + 1]) + (cr[r][2 * j] + cr[r][2 * j])) * 0.25f;
            }
            cbq[0][j] = quant((hb[0] + hb[1]) * 0.5f);
            crq[0][j] = quant((hr[0] + hr[1]) * 0.5f);
        }
    }

    if (full) {
#pragma unroll
        for (int r = 0; r < 2; ++r) store_row8(Yp + (size_t)(y0 + r) * W + x0, yq[r]);
        if (MODE == YUV_444) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                store_row8(Cbp + (size_t)(y0 + r) * W + x0, cbq[r]);
                store_row8(Crp + (size_t)(y0 + r) * W + x0, crq[r]);
            }
        } else {
            const size_t c = (size_t)by * Wc + x0 / 2;
            B4 ob, orr;
            ob.v = cbq[0][0] | cbq[0][1] << 8 | cbq[0][2] << 16 | cbq[0][3] << 24;
            orr.v = crq[0][0] | crq[0][1] << 8 | crq[0][2] << 16 | crq[0][3] << 24;
            *reinterpret_cast<B4*>(Cbp + c) = ob;
            *reinterpret_cast<B4*>(Crp + c) = orr;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i)
                if (x0 + i < W && y0 + r < H) {
                    const size_t p = (size_t)(y0 + r) * W + x0 + i;
                    Yp[p] = (uint8_t)yq[r][i];
                    if (MODE == YUV_444) { Cbp[p] = (uint8_t)cbq[r][i]; Crp[p] = (uint8_t)crq[r][i]; }
                }
        if (MODE != YUV_444) {
#pragma unroll
            for (int j = 0; j < YUV_BW / 2; ++j)
                if (x0 / 2 + j < Wc) {
                    const size_t c = (size_t)by * Wc + x0 / 2 + j;
                    Cbp[c] = (uint8_t)cbq[0][j]; Crp[c] = (uint8_t)crq[0][j];
                }
        }
    }
}

}  // namespace fav
