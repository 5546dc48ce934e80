// kernels_yuv.hip -- 8-bit YCbCr planes (the payload of a YUV4MPEG2 frame) <-> RGB: what stands in front of and behind the frame loop
// when fav_stylize reads and writes video streams (-input_y4m / -output_y4m) instead of PPM and PNG files.
//
//   frame   plane Y [H][W], then Cb, then Cr, contiguous, 8 bits per sample; chroma planes [H][W] (4:4:4) or [ceil(H/2)][ceil(W/2)]
//           (4:2:0, a missing partner of an odd size is the replicated edge sample -- the pyramid's rule in kernels_flow.hip)
//   matrix  (Kr, Kb) of BT.601 / BT.709, Kg = 1 - Kr - Kb; full range sy = sc = 1, oy = 0; limited sy = 219/255, sc = 224/255, oy = 16;
//           every constant is formed in double and rounded ONCE to fp32 (yuv_constants)
//   encode  y = (Kr R + Kg G) + Kb B;  Y = y sy + oy;  Cb = (B - y) (sc / (2 (1 - Kb))) + 128;  Cr = (R - y) (sc / (2 (1 - Kr))) + 128
//           4:2:0 reduces the UNQUANTISED Cb, Cr:  centre siting ((c00 + c01) + (c10 + c11)) / 4 over the 2 x 2 block;  left siting
//           h = ((l + r) + (c + c)) / 4 per row at the even column (neighbours clamped to the image), then (h0 + h1) / 2
//   decode  4:2:0 chroma is interpolated bilinearly to the luma grid (weights 1/4, 3/4; left siting: even columns take the sample, odd
//           ones the mean of two; indices clamped) -- exact in fp32 on 8-bit samples -- then y = (Y - oy) / sy, R = y + kR cr,
//           B = y + kB cb, G = (y - kGr cr) - kGb cb
//   bytes   floor(x + 0.5) clamped to [0, 255]
// All arithmetic is fp32 in the order written; the unit is compiled with -ffp-contract=off, and tests/util/yuv_model.py restates it in
// numpy: the kernels are held to that model byte for byte.
//
// Shape: no LDS.  A lane owns 2 rows x 8 columns of pixels, so it forms its own 4 (4:2:0) chroma samples: a row of the block is ONE
// 8-byte access in a byte plane, 24 bytes in the interleaved RGB image, 32 bytes in an fp32 plane, and a 4:2:0 chroma row one 4-byte
// access.  A plane's rows start at any byte (W is arbitrary), so the vector accesses are declared unaligned; the hardware takes them.
// A block that the frame does not fill (the last columns when W is no multiple of 8, the last row when H is odd) goes sample by sample
// with clamped reads -- which IS the replicated edge -- and guarded byte stores: nothing outside the frame's bytes is read or written.
// Pure streaming: 12 B/px in for the fp32 encode, 3 in / 1.5 out for the byte encode, the reverse for the decode.
// The constants, the byte rules and the encode's block live in yuv_device.h: kernels_color.hip encodes through the same block.
#include "yuv_device.h"

namespace fav {

namespace {

// [H][W][3] u8 or planar fp32 [3][H][W] (image.save's quantisation in front) -> the frame's planes: the lane's block of yuv_device.h
template <int MODE, bool FROM_F32>
__global__ __launch_bounds__(YUV_NT) void rgb_to_yuv_kernel(const uint8_t* __restrict__ rgb8, const float* __restrict__ rgbf, int W, int H, YuvK k,
                                                            uint8_t* __restrict__ yuv)
{
    if (FROM_F32) yuv_encode_block<MODE>(SrcF32{rgbf, W, (size_t)W * H}, W, H, k, yuv);
    else yuv_encode_block<MODE>(SrcRgb8{rgb8, W}, W, H, k, yuv);
}

// the frame's planes -> [H][W][3] u8 (the layout fav_stream_* takes as frame_rgb_hwc)
template <int MODE>
__global__ __launch_bounds__(YUV_NT) void yuv_to_rgb8_kernel(const uint8_t* __restrict__ yuv, int W, int H, YuvK k, uint8_t* __restrict__ rgb)
{
    const int nbx = (W + YUV_BW - 1) / YUV_BW, nby = (H + 1) / 2;
    const unsigned idx = blockIdx.x * YUV_NT + threadIdx.x;       // (W * H <= 2^28: the blocks of a frame number below 2^28)
    if (idx >= (unsigned)nbx * (unsigned)nby) return;
    const int by = (int)(idx / (unsigned)nbx), bx = (int)(idx - (unsigned)by * (unsigned)nbx);
    const int x0 = bx * YUV_BW, y0 = by * 2;
    const bool full = x0 + YUV_BW <= W && y0 + 2 <= H;
    const size_t plane = (size_t)W * H;
    const int Wc = MODE == YUV_444 ? W : (W + 1) / 2, Hc = MODE == YUV_444 ? H : (H + 1) / 2;
    const uint8_t* const Yp = yuv;
    const uint8_t* const Cbp = yuv + plane;
    const uint8_t* const Crp = Cbp + (size_t)Wc * Hc;

    float Y[2][YUV_BW], Cb[2][YUV_BW], Cr[2][YUV_BW];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const size_t p = (size_t)min(y0 + r, H - 1) * W;
        if (full) {
            const B8 v = *reinterpret_cast<const B8*>(Yp + p + x0);
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i) Y[r][i] = byte_of(v.v, i);
            if (MODE == YUV_444) {
                const B8 vb = *reinterpret_cast<const B8*>(Cbp + p + x0), vr = *reinterpret_cast<const B8*>(Crp + p + x0);
#pragma unroll
                for (int i = 0; i < YUV_BW; ++i) { Cb[r][i] = byte_of(vb.v, i); Cr[r][i] = byte_of(vr.v, i); }
            }
        } else {
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i) {
                const size_t q = p + min(x0 + i, W - 1);
                Y[r][i] = (float)Yp[q];
                if (MODE == YUV_444) { Cb[r][i] = (float)Cbp[q]; Cr[r][i] = (float)Crp[q]; }
            }
        }
    }
    if (MODE != YUV_444) {
        // chroma rows by - 1, by, by + 1 and columns x0/2 - 1 .. x0/2 + 4 of both planes, indices clamped to the plane
        const int cx0 = x0 / 2;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const uint8_t* const P = pl ? Crp : Cbp;
            float c[3][6];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const uint8_t* const row = P + (size_t)min(max(by - 1 + r, 0), Hc - 1) * Wc;
                c[r][0] = (float)row[max(cx0 - 1, 0)];
                c[r][5] = (float)row[min(cx0 + 4, Wc - 1)];
                if (full) {
                    const uint32_t v = reinterpret_cast<const B4*>(row + cx0)->v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) c[r][1 + i] = byte_of(&v, i);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) c[r][1 + i] = (float)row[min(cx0 + i, Wc - 1)];
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float v[6];       // vertical: row 2j takes 0.25 C[j-1] + 0.75 C[j], row 2j+1 takes 0.75 C[j] + 0.25 C[j+1]
#pragma unroll
                for (int i = 0; i < 6; ++i) v[i] = 0.25f * c[2 * r][i] + 0.75f * c[1][i];
                float* const out = pl ? Cr[r] : Cb[r];
#pragma unroll
                for (int j = 0; j < YUV_BW / 2; ++j) {
                    if (MODE == YUV_420_CENTER) {
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
            const float y = (Y[r][i] - k.oy) * k.isy, cb = Cb[r][i] - 128.f, cr = Cr[r][i] - 128.f;
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


}  // namespace

size_t yuv_frame_bytes(int W, int H, const fav_yuv_format& f)
{
    const size_t wc = f.chroma == FAV_YUV_444 ? W : (W + 1) / 2, hc = f.chroma == FAV_YUV_444 ? H : (H + 1) / 2;
    return (size_t)W * H + 2 * wc * hc;
}

int launch_yuv_to_rgb8(const uint8_t* yuv, int W, int H, const fav_yuv_format& f, uint8_t* rgb_hwc, hipStream_t st)
{
    const YuvK k = yuv_constants(f);
    const dim3 grid(yuv_grid(W, H)), block(YUV_NT);
    switch (yuv_mode(f)) {
    case YUV_420_CENTER: hipLaunchKernelGGL((yuv_to_rgb8_kernel<YUV_420_CENTER>), grid, block, 0, st, yuv, W, H, k, rgb_hwc); break;
    case YUV_420_LEFT: hipLaunchKernelGGL((yuv_to_rgb8_kernel<YUV_420_LEFT>), grid, block, 0, st, yuv, W, H, k, rgb_hwc); break;
    default: hipLaunchKernelGGL((yuv_to_rgb8_kernel<YUV_444>), grid, block, 0, st, yuv, W, H, k, rgb_hwc); break;
    }
    FAV_LAUNCH_CHECK("yuv_to_rgb8_kernel");
    return FAV_OK;
}

// exactly one of rgb_hwc / rgb_planar
int launch_rgb_to_yuv(const uint8_t* rgb_hwc, const float* rgb_planar, int W, int H, const fav_yuv_format& f, uint8_t* yuv, hipStream_t st)
{
    const YuvK k = yuv_constants(f);
    const dim3 grid(yuv_grid(W, H)), block(YUV_NT);
#define FAV_YUV_ENC(MODE_)                                                                                                              \
    if (rgb_planar) hipLaunchKernelGGL((rgb_to_yuv_kernel<MODE_, true>), grid, block, 0, st, rgb_hwc, rgb_planar, W, H, k, yuv);       \
    else hipLaunchKernelGGL((rgb_to_yuv_kernel<MODE_, false>), grid, block, 0, st, rgb_hwc, rgb_planar, W, H, k, yuv)
    switch (yuv_mode(f)) {
    case YUV_420_CENTER: FAV_YUV_ENC(YUV_420_CENTER); break;
    case YUV_420_LEFT: FAV_YUV_ENC(YUV_420_LEFT); break;
    default: FAV_YUV_ENC(YUV_444); break;
    }
#undef FAV_YUV_ENC
    FAV_LAUNCH_CHECK("rgb_to_yuv_kernel");
    return FAV_OK;
}

}  // namespace fav
