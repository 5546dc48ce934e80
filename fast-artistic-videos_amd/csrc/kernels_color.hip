// kernels_color.hip -- fav_stylize -original_colors: the stylised frame's luminance on the input frame's colours (the luminance transfer
// of Gatys et al., "Preserving color in neural artistic style transfer"), where the frame leaves: the recurrent state is not touched.
//
//   S       the stylised frame's bytes: image.save's quantisation of the state (clamp to [0, 1], x255, truncate -- save_byte, the one
//           fav_png_encode_f32 and fav_rgb_f32_to_yuv apply);  O  the original frame's bytes, [H][W][3] u8
//   pixel   ys = (Kr Sr + Kg Sg) + Kb Sb;  yo = (Kr Or + Kg Og) + Kb Ob;  d = ys - yo;  Pc = clamp(floor((Oc + d) + 0.5), 0, 255), c = R, G, B
//           (Kr, Kb) of BT.601 / BT.709, Kg = 1 - Kr - Kb, formed in double and rounded once (yuv_constants).  No range scaling enters:
//           the transfer happens on full-range RGB, a Y4M output's range is applied afterwards by the ordinary conversion
//   planes  the conversion of P's BYTES by the block of yuv_device.h -- not Y of S next to the chroma of O: both output routes describe
//           one image, and fav_color_transfer_yuv gives the bytes of fav_rgb8_to_yuv(fav_color_transfer_rgb8(...))
// All arithmetic is fp32 in the order written; the unit is compiled with -ffp-contract=off, and tests/util/color_model.py restates it in
// numpy: the kernels are held to that model byte for byte.
//
// Shape: that of kernels_yuv.hip.  No LDS; a lane owns 2 rows x 8 columns; a row of the block is three 32-byte loads from the state's
// planes and one 24-byte load from O, all declared unaligned (any W, any pointer offset); a block that the frame does not fill goes
// pixel by pixel with clamped reads and guarded byte stores: nothing outside the frame's bytes is read or written.
// Pure streaming: 15 B/px in; 3 B/px out for the image, 1.5 or 3 for the planes.
#include "yuv_device.h"

namespace fav {

namespace {

// P as a source of the encode block: the pixel formed in registers from the state and the original frame
struct SrcTransfer {
    SrcF32 s; SrcRgb8 o; float kr, kg, kb;
    __device__ __forceinline__ void transfer(float Sr, float Sg, float Sb, float& R, float& G, float& B) const      // in: O, out: P
    {
        const float ys = (kr * Sr + kg * Sg) + kb * Sb;
        const float yo = (kr * R + kg * G) + kb * B;
        const float d = ys - yo;
        R = quantf(R + d); G = quantf(G + d); B = quantf(B + d);
    }
    __device__ __forceinline__ void pixel(int x, int y, float& R, float& G, float& B) const
    {
        float Sr, Sg, Sb;
        s.pixel(x, y, Sr, Sg, Sb);
        o.pixel(x, y, R, G, B);
        transfer(Sr, Sg, Sb, R, G, B);
    }
    __device__ __forceinline__ void row8(int x0, int y, float* R, float* G, float* B) const
    {
        float Sr[YUV_BW], Sg[YUV_BW], Sb[YUV_BW];
        s.row8(x0, y, Sr, Sg, Sb);
        o.row8(x0, y, R, G, B);
#pragma unroll
        for (int i = 0; i < YUV_BW; ++i) transfer(Sr[i], Sg[i], Sb[i], R[i], G[i], B[i]);
    }
};

// state planes [3][H][W] fp32 + O -> P [H][W][3] u8
__global__ __launch_bounds__(YUV_NT) void color_transfer_rgb8_kernel(const float* __restrict__ state, const uint8_t* __restrict__ orig, int W, int H,
                                                                     float kr, float kg, float kb, uint8_t* __restrict__ out)
{
    int bx, by;
    if (!yuv_block_of(W, H, bx, by)) return;
    const int x0 = bx * YUV_BW, y0 = by * 2;
    const bool full = x0 + YUV_BW <= W && y0 + 2 <= H;
    const SrcTransfer src{SrcF32{state, W, (size_t)W * H}, SrcRgb8{orig, W}, kr, kg, kb};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        if (full) {
            float R[YUV_BW], G[YUV_BW], B[YUV_BW];
            src.row8(x0, y, R, G, B);
            uint32_t q[3 * YUV_BW];
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i) { q[3 * i] = (uint32_t)R[i]; q[3 * i + 1] = (uint32_t)G[i]; q[3 * i + 2] = (uint32_t)B[i]; }
            B24 o;
#pragma unroll
            for (int w = 0; w < 6; ++w) o.v[w] = q[4 * w] | q[4 * w + 1] << 8 | q[4 * w + 2] << 16 | q[4 * w + 3] << 24;
            *reinterpret_cast<B24*>(out + 3 * ((size_t)y * W + x0)) = o;
        } else if (y < H) {
#pragma unroll
            for (int i = 0; i < YUV_BW; ++i)
                if (x0 + i < W) {
                    float R, G, B;
                    src.pixel(x0 + i, y, R, G, B);
                    uint8_t* const d = out + 3 * ((size_t)y * W + x0 + i);
                    d[0] = (uint8_t)R; d[1] = (uint8_t)G; d[2] = (uint8_t)B;
                }
        }
    }
}

// the same pixel, fused with the RGB -> YCbCr encode: P never exists in memory
template <int MODE>
__global__ __launch_bounds__(YUV_NT) void color_transfer_yuv_kernel(const float* __restrict__ state, const uint8_t* __restrict__ orig, int W, int H, YuvK k,
                                                                    uint8_t* __restrict__ yuv)
{
    yuv_encode_block<MODE>(SrcTransfer{SrcF32{state, W, (size_t)W * H}, SrcRgb8{orig, W}, k.kr, k.kg, k.kb}, W, H, k, yuv);
}

}  // namespace

int launch_color_transfer_rgb8(const float* state, const uint8_t* orig_hwc, int W, int H, int matrix, uint8_t* out_hwc, hipStream_t st)
{
    const YuvK k = yuv_constants(fav_yuv_format{FAV_YUV_444, FAV_YUV_SITING_CENTER, matrix, 1});      // (Kr, Kg, Kb depend on the matrix alone)
    hipLaunchKernelGGL(color_transfer_rgb8_kernel, dim3(yuv_grid(W, H)), dim3(YUV_NT), 0, st, state, orig_hwc, W, H, k.kr, k.kg, k.kb, out_hwc);
    FAV_LAUNCH_CHECK("color_transfer_rgb8_kernel");
    return FAV_OK;
}

int launch_color_transfer_yuv(const float* state, const uint8_t* orig_hwc, int W, int H, const fav_yuv_format& f, uint8_t* yuv, hipStream_t st)
{
    const YuvK k = yuv_constants(f);
    const dim3 grid(yuv_grid(W, H)), block(YUV_NT);
    switch (yuv_mode(f)) {
    case YUV_420_CENTER: hipLaunchKernelGGL((color_transfer_yuv_kernel<YUV_420_CENTER>), grid, block, 0, st, state, orig_hwc, W, H, k, yuv); break;
    case YUV_420_LEFT: hipLaunchKernelGGL((color_transfer_yuv_kernel<YUV_420_LEFT>), grid, block, 0, st, state, orig_hwc, W, H, k, yuv); break;
    default: hipLaunchKernelGGL((color_transfer_yuv_kernel<YUV_444>), grid, block, 0, st, state, orig_hwc, W, H, k, yuv); break;
    }
    FAV_LAUNCH_CHECK("color_transfer_yuv_kernel");
    return FAV_OK;
}

}  // namespace fav
