// kernels_yuv_layout.hip -- YCbCr planes of every layout of include/fav_yuv.h <-> RGB: 4:2:0, 4:2:2 and 4:4:4 at 8 .. 16 bits per sample.
// What fav_stylize runs in front of and behind the frame loop when the Y4M stream is 10-bit (C420p10: phones, cameras) or 4:2:2 (C422,
// C422p10: broadcast, ProRes).  kernels_yuv.hip says what the arithmetic is and why the block has its shape; this unit keeps both:
//
//   arithmetic  that of kernels_yuv.hip with the depth D in the constants (yuv_layout_constants): SY, OY, SC scaled by 2^(D-8) (limited)
//               or (2^D - 1)/255 (full), chroma offset 2^(D-1), samples clamped to [0, 2^D - 1].  An input sample is the 16-bit number it
//               is.  4:2:0 interpolates / reduces as there -- the weights 1/4, 3/4, 1/2 stay exact in fp32 on 16-bit samples (18 of 24
//               mantissa bits), so the order of the axes still does not matter; 4:2:2 is the horizontal rule of each siting alone.
//   depth 8     4:2:0 and 4:4:4 at depth 8 ARE kernels_yuv.hip's kernels: the launchers below hand them over, so those bytes are today's
//               by construction.  Only 4:2:2 is instantiated on byte samples here.
//   fp32 source depth 8: image.save's truncation in front (SrcF32), as in kernels_yuv.hip; deeper: the floats enter unquantised (SrcF32Raw)
//   shape       no LDS; a lane owns 2 rows x 8 columns and forms its own chroma: 1 x 4 (4:2:0), 2 x 4 (4:2:2), 2 x 8 (4:4:4).  A row of
//               8 two-byte samples is ONE 16-byte access, a chroma row of 4 one 8-byte access, declared unaligned (a plane starts at any
//               byte, odd ones included).  The decode reads the chroma of its neighbours as single samples.  A block the frame does not
//               fill goes sample by sample with clamped reads and guarded stores: nothing outside the frame's bytes is read or written.
// -ffp-contract=off; tests/util/yuv_layout_model.py restates the arithmetic and the kernels are held to it sample for sample.
#include "yuv_layout_device.h"

namespace fav {

namespace {

enum { SRC_RGB8 = 0, SRC_F32_SAVED = 1, SRC_F32_RAW = 2 };

template <int MODE, class T, int SRC>
__global__ __launch_bounds__(YUV_NT) void rgb_to_yuv_layout_kernel(const uint8_t* __restrict__ rgb8, const float* __restrict__ rgbf, int W, int H, YuvLK k,
                                                                   uint8_t* __restrict__ yuv)
{
    if (SRC == SRC_RGB8) yuv_layout_encode_block<MODE, T>(SrcRgb8{rgb8, W}, W, H, k, yuv);
    else if (SRC == SRC_F32_SAVED) yuv_layout_encode_block<MODE, T>(SrcF32{rgbf, W, (size_t)W * H}, W, H, k, yuv);
    else yuv_layout_encode_block<MODE, T>(SrcF32Raw{rgbf, W, (size_t)W * H}, W, H, k, yuv);
}

// the frame's planes -> [H][W][3] u8
template <int MODE, class T>
__global__ __launch_bounds__(YUV_NT) void yuv_layout_to_rgb8_kernel(const uint8_t* __restrict__ yuv, int W, int H, YuvLK k, uint8_t* __restrict__ rgb)
{
    using S = Smp<T>;
    int bx, by;
    if (!yuv_block_of(W, H, bx, by)) return;
    const int x0 = bx * YUV_BW, y0 = by * 2;
    const bool full = x0 + YUV_BW <= W && y0 + 2 <= H;
    const size_t plane = (size_t)W * H;
    const int Wc = MODE == YL_444 ? W : (W + 1) / 2, Hc = yl_is_420(MODE) ? (H + 1) / 2 : H;
    const uint8_t* const Yp = yuv;
    const uint8_t* const Cbp = yuv + plane * S::BYTES;
    const uint8_t* const Crp = Cbp + (size_t)Wc * Hc * S::BYTES;

    float Y[2][YUV_BW], Cb[2][YUV_BW], Cr[2][YUV_BW];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const size_t p = (size_t)min(y0 + r, H - 1) * W;
        if (full) {
            S::ld_row8(Yp, p + x0, Y[r]);
            if (MODE == YL_444) { S::ld_row8(Cbp, p + x0, Cb[r]); S::ld_row8(Crp, p + x0, Cr[r]); }
        } else {
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i) {
                const size_t q = p + min(x0 + i, W - 1);
                Y[r][i] = S::ld(Yp, q);
                if (MODE == YL_444) { Cb[r][i] = S::ld(Cbp, q); Cr[r][i] = S::ld(Crp, q); }
            }
        }
    }
    if (MODE != YL_444) {
        // 4:2:0: chroma rows by - 1, by, by + 1; 4:2:2: the block's own two rows.  Columns x0/2 - 1 .. x0/2 + 4, indices clamped to the plane.
        constexpr int NR = yl_is_420(MODE) ? 3 : 2;
        const int cx0 = x0 / 2;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const uint8_t* const P = pl ? Crp : Cbp;
            float c[NR][6];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int cy = yl_is_420(MODE) ? min(max(by - 1 + r, 0), Hc - 1) : min(y0 + r, Hc - 1);
                const size_t row = (size_t)cy * Wc;
                c[r][0] = S::ld(P, row + max(cx0 - 1, 0));
                c[r][5] = S::ld(P, row + min(cx0 + 4, Wc - 1));
                if (full) S::ld_row4(P, row + cx0, &c[r][1]);
                else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) c[r][1 + i] = S::ld(P, row + min(cx0 + i, Wc - 1));
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float v[6];       // 4:2:0, vertical: row 2j takes 0.25 C[j-1] + 0.75 C[j], row 2j+1 takes 0.75 C[j] + 0.25 C[j+1]
#pragma unroll
                for (int i = 0; i < 6; ++i) v[i] = yl_is_420(MODE) ? 0.25f * c[yl_is_420(MODE) ? 2 * r : r][i] + 0.75f * c[1][i] : c[r][i];
                float* const out = pl ? Cr[r] : Cb[r];
#pragma unroll
                for (int j = 0; j < YUV_BW / 2; ++j) {
                    if (!yl_is_left(MODE)) {
                        out[2 * j] = 0.25f * v[j] + 0.75f * v[j + 1];
                        out[2 * j + 1] = 0.25f * v[j + 2] + 0.75f * v[j + 1];
                    } else {
                        out[2 * j] = v[j + 1];
                        out[2 * j + 1] = 0.5f * (v[j + 1] + v[j + 2]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint32_t q[3 * YUV_BW];
#pragma unroll
        for (int i = 0; i < YUV_BW; ++i) {
            const float y = (Y[r][i] - k.oy) * k.isy, cb = Cb[r][i] - k.oc, cr = Cr[r][i] - k.oc;
            q[3 * i] = quant(y + k.kR * cr);
            q[3 * i + 1] = quant((y - k.kGr * cr) - k.kGb * cb);
            q[3 * i + 2] = quant(y + k.kB * cb);
        }
        if (full) {
            B24 o;
#pragma unroll
            for (int w = 0; w < 6; ++w) o.v[w] = q[4 * w] | q[4 * w + 1] << 8 | q[4 * w + 2] << 16 | q[4 * w + 3] << 24;
            *reinterpret_cast<B24*>(rgb + 3 * ((size_t)(y0 + r) * W + x0)) = o;
        } else if (y0 + r < H) {
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i)
                if (x0 + i < W) {
                    uint8_t* const d = rgb + 3 * ((size_t)(y0 + r) * W + x0 + i);
                    d[0] = (uint8_t)q[3 * i]; d[1] = (uint8_t)q[3 * i + 1]; d[2] = (uint8_t)q[3 * i + 2];
                }
        }
    }
}

inline fav_yuv_format format_of(const fav_yuv_layout& l) { return fav_yuv_format{l.chroma, l.siting, l.matrix, l.full_range}; }
inline bool todays_kernel(const fav_yuv_layout& l) { return l.depth == 8 && l.chroma != FAV_YUV_422; }

}  // namespace

size_t yuv_layout_frame_bytes(int W, int H, const fav_yuv_layout& l)
{
    const size_t wc = l.chroma == FAV_YUV_444 ? W : (W + 1) / 2, hc = l.chroma == FAV_YUV_420 ? (H + 1) / 2 : H;
    return ((size_t)W * H + 2 * wc * hc) * (l.depth > 8 ? 2 : 1);
}

int launch_yuv_layout_to_rgb8(const void* yuv_, int W, int H, const fav_yuv_layout& l, uint8_t* rgb_hwc, hipStream_t st)
{
    const uint8_t* const yuv = static_cast<const uint8_t*>(yuv_);
    if (todays_kernel(l)) return launch_yuv_to_rgb8(yuv, W, H, format_of(l), rgb_hwc, st);
    const YuvLK k = yuv_layout_constants(l);
    const dim3 grid(yuv_grid(W, H)), block(YUV_NT);
#define FAV_YL_DEC(MODE_, T_) hipLaunchKernelGGL((yuv_layout_to_rgb8_kernel<MODE_, T_>), grid, block, 0, st, yuv, W, H, k, rgb_hwc)
    const int mode = yuv_layout_mode(l);
    if (l.depth == 8) {
        if (mode == YL_422_LEFT) FAV_YL_DEC(YL_422_LEFT, uint8_t); else FAV_YL_DEC(YL_422_CENTER, uint8_t);
    } else switch (mode) {
    case YL_420_CENTER: FAV_YL_DEC(YL_420_CENTER, uint16_t); break;
    case YL_420_LEFT: FAV_YL_DEC(YL_420_LEFT, uint16_t); break;
    case YL_422_CENTER: FAV_YL_DEC(YL_422_CENTER, uint16_t); break;
    case YL_422_LEFT: FAV_YL_DEC(YL_422_LEFT, uint16_t); break;
    default: FAV_YL_DEC(YL_444, uint16_t); break;
    }
#undef FAV_YL_DEC
    FAV_LAUNCH_CHECK("yuv_layout_to_rgb8_kernel");
    return FAV_OK;
}

// exactly one of rgb_hwc / rgb_planar
int launch_rgb_to_yuv_layout(const uint8_t* rgb_hwc, const float* rgb_planar, int W, int H, const fav_yuv_layout& l, void* yuv_, hipStream_t st)
{
    uint8_t* const yuv = static_cast<uint8_t*>(yuv_);
    if (todays_kernel(l)) return launch_rgb_to_yuv(rgb_hwc, rgb_planar, W, H, format_of(l), yuv, st);
    const YuvLK k = yuv_layout_constants(l);
    const dim3 grid(yuv_grid(W, H)), block(YUV_NT);
    // the fp32 source: truncated like image.save at depth 8, unquantised above
#define FAV_YL_ENC(MODE_, T_, F32_)                                                                                                             \
    if (rgb_planar) hipLaunchKernelGGL((rgb_to_yuv_layout_kernel<MODE_, T_, F32_>), grid, block, 0, st, rgb_hwc, rgb_planar, W, H, k, yuv);    \
    else hipLaunchKernelGGL((rgb_to_yuv_layout_kernel<MODE_, T_, SRC_RGB8>), grid, block, 0, st, rgb_hwc, rgb_planar, W, H, k, yuv)
    const int mode = yuv_layout_mode(l);
    if (l.depth == 8) {
        if (mode == YL_422_LEFT) { FAV_YL_ENC(YL_422_LEFT, uint8_t, SRC_F32_SAVED); } else { FAV_YL_ENC(YL_422_CENTER, uint8_t, SRC_F32_SAVED); }
    } else switch (mode) {
    case YL_420_CENTER: FAV_YL_ENC(YL_420_CENTER, uint16_t, SRC_F32_RAW); break;
    case YL_420_LEFT: FAV_YL_ENC(YL_420_LEFT, uint16_t, SRC_F32_RAW); break;
    case YL_422_CENTER: FAV_YL_ENC(YL_422_CENTER, uint16_t, SRC_F32_RAW); break;
    case YL_422_LEFT: FAV_YL_ENC(YL_422_LEFT, uint16_t, SRC_F32_RAW); break;
    default: FAV_YL_ENC(YL_444, uint16_t, SRC_F32_RAW); break;
    }
#undef FAV_YL_ENC
    FAV_LAUNCH_CHECK("rgb_to_yuv_layout_kernel");
    return FAV_OK;
}

}  // namespace fav
