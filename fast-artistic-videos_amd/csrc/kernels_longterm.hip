// kernels_longterm.hip -- input assembly with LONG-TERM priors (Ruder, Dosovitskiy, Brox: "Artistic style transfer for videos", 2016,
// section 4.2): the K-prior form of prep_input_kernel (kernels_frame.hip).  The stylised frames i - d_k of K distances (ascending, d_0 = 1)
// are each warped to frame i by their own backward flow; a pixel takes each prior with the weight
//     w_k = max(c_k - sum_{j < k} c_j, 0)              c_k: the eroded certainty of distance d_k
// i.e. the nearest frame in which it was visible, and the merged certainty C = sum_k w_k <= 1 is what the network sees in channel 6.
// One lane per pixel of the padded NHWC8 input, the reflection folded in, as prep_input_kernel; HBM-bound.  With K = 1 the eight floats
// are prep_pixel's, bit for bit.  Compiled with -ffp-contract=off: tests/util/long_term_model.py restates the arithmetic in this order.
#include "fav_internal.h"
#include "frame_taps.h"

namespace fav {
namespace {

// the K priors of a frame, by value in the kernel arguments: no pointer table in device memory, nothing to upload per frame
struct LongTermArgs {
    const float* state[FAV_LONG_TERM_MAX];       // [3][Hs][Ws] stylised frame i - d_k
    const float2* flo[FAV_LONG_TERM_MAX];        // [H][W] backward flow: A = frame i, B = frame i - d_k
    const float* cert[FAV_LONG_TERM_MAX];        // [H][W] eroded certainty of that flow
};

__global__ __launch_bounds__(256) void longterm_prep_kernel(const uint8_t* frame_hwc, LongTermArgs a, int K, int Hs, int Ws, int border, int H,
                                                            int W, int pad, float* in8, float* cert_out, int fill_random, unsigned seed, unsigned index)
{
    // image.load: byte / 255 -- the 256 possible quotients are formed once per block (prep_input_kernel)
    __shared__ float byte01[256];
    byte01[threadIdx.x] = (float)threadIdx.x / 255.f;
    __syncthreads();
    const int Wp = W + 2 * pad;
    const int yp = blockIdx.y, xp = blockIdx.x * 256 + threadIdx.x;
    if (xp >= Wp) return;
    const int y = reflect(yp - pad, H), x = reflect(xp - pad, W);
    const size_t i = (size_t)y * W + x;
    const uint8_t* px = frame_hwc + i * 3;
    const float rgb[3] = {byte01[px[0]], byte01[px[1]], byte01[px[2]]};
    float4 lo, hi;
    lo.x = rgb[2] * 255.f - 103.939f;
    lo.y = rgb[1] * 255.f - 116.779f;
    lo.z = rgb[0] * 255.f - 123.68f;
    const size_t ns = (size_t)Hs * Ws;
    float used = 0.f, C = 0.f, ab = 0.f, ag = 0.f, ar = 0.f;
#pragma unroll
    for (int k = 0; k < FAV_LONG_TERM_MAX; ++k) {
        if (k >= K) break;
        const float c = a.cert[k][i];
        const float w = fmaxf(c - used, 0.f);
        used = used + c;
        C = C + w;
        if (w == 0.f) continue;                      // the common case beyond distance 1: no gather, and nothing of this prior enters
        const float2 f = a.flo[k][i];                                   // .flo payload: (u, v) = (dx, dy)
        const Taps t = make_taps(border, f.y + (float)y, f.x + (float)x, Hs, Ws);
        const float* st = a.state[k];
        const float wr = sample_pairs(st, t), wg = sample_pairs(st + ns, t), wb = sample_pairs(st + 2 * ns, t);
        ab += (wb * 255.f - 103.939f) * w;
        ag += (wg * 255.f - 116.779f) * w;
        ar += (wr * 255.f - 123.68f) * w;
    }
    // generate_fill (core.lua:108-117) under the MERGED certainty: 0 (vgg-mean) or pre(u) * (1 - C)
    float fb = 0.f, fg = 0.f, fr = 0.f;
    if (fill_random) {
        const float cinv = (C + -1.f) * -1.f;
        fb = (fill_uniform(seed, index, 2, y, x) * 255.f - 103.939f) * cinv;
        fg = (fill_uniform(seed, index, 1, y, x) * 255.f - 116.779f) * cinv;
        fr = (fill_uniform(seed, index, 0, y, x) * 255.f - 123.68f) * cinv;
    }
    lo.w = fb + ab;                                                     // torch.add(fill, prev_warped_masked), core:169
    hi.x = fg + ag;
    hi.y = fr + ar;
    hi.z = C;
    hi.w = 0.f;
    float4* o = reinterpret_cast<float4*>(in8 + ((size_t)yp * Wp + xp) * 8);
    o[0] = lo; o[1] = hi;
    if (cert_out && yp - pad == y && xp - pad == x) cert_out[i] = C;    // the pixel's own place, not its reflections
}

}  // namespace

int launch_longterm_prep(const uint8_t* frame_hwc, int K, const float* const* states, int Hs, int Ws, const float* const* backward_flo,
                         const float* const* cert, int border, int H, int W, int pad, float* in8, float* cert_out, hipStream_t st,
                         int fill_random, unsigned seed, unsigned index)
{
    FAV_REQUIRE(K >= 1 && K <= FAV_LONG_TERM_MAX, "long-term input assembly: %d priors (1..%d)", K, FAV_LONG_TERM_MAX);
    FAV_REQUIRE(pad >= 0 && pad < H && pad < W && Hs >= 1 && Ws >= 1, "long-term input assembly: needs 0 <= pad < H, W and a non-empty state");
    LongTermArgs a{};
    for (int k = 0; k < K; ++k) {
        a.state[k] = states[k]; a.flo[k] = reinterpret_cast<const float2*>(backward_flo[k]); a.cert[k] = cert[k];
    }
    hipLaunchKernelGGL(longterm_prep_kernel, dim3((W + 2 * pad + 255) / 256, H + 2 * pad), dim3(256), 0, st, frame_hwc, a, K, Hs, Ws, border,
                       H, W, pad, in8, cert_out, fill_random, seed, index);
    FAV_LAUNCH_CHECK("longterm_prep_kernel");
    return FAV_OK;
}

}  // namespace fav
