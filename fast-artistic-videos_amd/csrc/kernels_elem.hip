// kernels_elem.hip -- the elementwise kernels around the convolutions (InstanceNorm finalize and statistics, residual join, padding,
// layout conversion) and their launch wrappers.
#include <algorithm>

#include "fav_internal.h"
#include "conv_device.h"

namespace fav {

// ------------------------------------------------------------------------------------------------
// InstanceNorm finalize: merge per-tile (mean, M2) in fp64 (Chan et al.), emit scale/shift.
// InstanceNormalization.lua:33-53: biased variance, eps inside the sqrt.
// ------------------------------------------------------------------------------------------------
namespace {

// One pass over the per-tile (mean, M2, count) partials in fp64:  mean = sum n_b mean_b / M,  var = (sum M2_b + sum n_b mean_b^2) / M
// - mean^2 (biased).  The cancellation in the last step costs (mean^2 / var) ulps of fp64 -- far below the fp32 result's own
// rounding -- and saves the second dependent sweep + block reduction of the textbook two-pass merge: this kernel is pure
// latency (16 launches per frame), not bandwidth.  (Measured and dropped, profiles/r02p_*: blocks of 16 channels x 64 rows with
// line-coalesced reads and four loads in flight per thread -- 6.2 us against 5.2 us for this form: the launch plus ONE round trip
// to memory for data another XCD's L2 has just written back is what the 5 us are made of, not the read pattern.)
__global__ __launch_bounds__(256) void in_finalize_kernel(const float2* partials, const int* counts, int mblocks, int M, int bp,
                                                          int Cpitch, const float* gamma, const float* beta,
                                                          float eps, float* scale, float* shift)
{
    __shared__ double sh[8];
    const int c = blockIdx.x, t = threadIdx.x;
    double s1 = 0, s2 = 0;
    float gq = 1.f, bq = 0.f;
    if (t == 0) { gq = gamma ? gamma[c] : 1.f; bq = beta ? beta[c] : 0.f; }      // requested before the sweep, used after it
    // four independent rows per thread in flight (one batch covers 1024 partial rows: a single round trip to memory for every layer
    // of the 1280x720 network; a rolled loop waits for each row before it asks for the next)
    for (int b0 = t; b0 < mblocks; b0 += 1024) {
        float2 pr[4]; int nb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = b0 + 256 * k, bc = min(b, mblocks - 1);
            pr[k] = partials[(size_t)bc * Cpitch + c];
            nb[k] = b < mblocks ? (counts ? counts[bc] : min(bp, M - bc * bp)) : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double n = (double)nb[k], mu = (double)pr[k].x;
            s1 += n * mu;
            s2 += (nb[k] ? (double)pr[k].y : 0.0) + n * mu * mu;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if ((t & 63) == 0) { sh[2 * (t >> 6)] = s1; sh[2 * (t >> 6) + 1] = s2; }
    __syncthreads();
    if (t == 0) {
        const double a = ((sh[0] + sh[2]) + sh[4]) + sh[6], q = ((sh[1] + sh[3]) + sh[5]) + sh[7];
        const double mean = a / (double)M;
        double var = q / (double)M - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const double g = (double)gq, bt = (double)bq;
        const double sc = g / sqrt(var + (double)eps);
        scale[c] = (float)sc;
        shift[c] = (float)(bt - mean * sc);
    }
}

__device__ __forceinline__ float4 apply_affine_g(float4 v, const Affine& a, int c)
{
    if (a.stages >= 1) {
        v = affine4(v, a.scale1 + c, a.shift1 + c, a.relu1);
        if (a.stages >= 2) v = affine4(v, a.scale2 + c, a.shift2 + c, a.relu2);
    }
    return v;
}

// statistics of t(x) over [M][C]: one block per 128 pixels.  NPT > 0: the block's elements stay in registers between the mean
// and the M2 sweep (NPT = 128 / (256 / (C / 4)) float4 per thread: 8 for C = 64, 16 for C = 128) -- one read of the tensor
// instead of two; NPT = 0: any channel count, the tile is read twice.
template <int NPT>
__global__ __launch_bounds__(256) void stats_kernel(const float* x, int M, int C, const Affine a, float2* partials)
{
    __shared__ float red[1024];
    __shared__ float mean_s[1024];
    const int t = threadIdx.x;
    const int groups = C >> 2;                 // float4 groups per pixel
    const int nl = 256 / groups;               // pixel lanes
    const int g = t % groups, pl = t / groups;
    const int m0 = blockIdx.x * 128;
    const int cnt = min(128, M - m0);
    const bool active = pl < nl;
    float4 s = make_float4(0, 0, 0, 0);
    float4 keep[NPT > 0 ? NPT : 1];
    if (NPT > 0) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int pix = pl + i * nl;
            float4 v = make_float4(0, 0, 0, 0);
            if (pix < cnt) { v = *reinterpret_cast<const float4*>(x + (size_t)(m0 + pix) * C + 4 * g); v = apply_affine_g(v, a, 4 * g); }
            keep[i] = v;
        }
#pragma unroll
        for (int i = 0; i < NPT; ++i) { s.x += keep[i].x; s.y += keep[i].y; s.z += keep[i].z; s.w += keep[i].w; }      // (elements past cnt are zeros)
    } else if (active)
        for (int pix = pl; pix < cnt; pix += nl) {
            float4 v = *reinterpret_cast<const float4*>(x + (size_t)(m0 + pix) * C + 4 * g);
            v = apply_affine_g(v, a, 4 * g);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    if (active) *reinterpret_cast<float4*>(red + pl * C + 4 * g) = s;
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        float r = 0;
        for (int i = 0; i < nl; ++i) r += red[i * C + c];
        mean_s[c] = r / (float)cnt;
    }
    __syncthreads();
    float4 q = make_float4(0, 0, 0, 0);
    if (active) {
        const float4 mu = *reinterpret_cast<const float4*>(mean_s + 4 * g);
        if (NPT > 0) {
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const float4 v = keep[i];
                const float dx = v.x - mu.x, dy = v.y - mu.y, dz = v.z - mu.z, dw = v.w - mu.w;
                if (pl + i * nl < cnt) { q.x = fmaf(dx, dx, q.x); q.y = fmaf(dy, dy, q.y); q.z = fmaf(dz, dz, q.z); q.w = fmaf(dw, dw, q.w); }
            }
        } else
            for (int pix = pl; pix < cnt; pix += nl) {
                float4 v = *reinterpret_cast<const float4*>(x + (size_t)(m0 + pix) * C + 4 * g);
                v = apply_affine_g(v, a, 4 * g);
                const float dx = v.x - mu.x, dy = v.y - mu.y, dz = v.z - mu.z, dw = v.w - mu.w;
                q.x = fmaf(dx, dx, q.x); q.y = fmaf(dy, dy, q.y); q.z = fmaf(dz, dz, q.z); q.w = fmaf(dw, dw, q.w);
            }
        *reinterpret_cast<float4*>(red + pl * C + 4 * g) = q;
    }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        float r = 0;
        for (int i = 0; i < nl; ++i) r += red[i * C + c];
        partials[(size_t)blockIdx.x * C + c] = make_float2(mean_s[c], r);
    }
}

// residual join: nn.CAddTable of (IN(conv_b) , ShaveImage(skip))  -- models_video.lua:41-53.
// res_add_stats_kernel: the join feeds an InstanceNorm (directly or through a nearest upsample, which leaves mean and biased
// variance unchanged: the R128 -> U2 -> IN tail of models_video.lua:94-98): one block = one row segment of up to 128 pixels, and
// the same pass yields that norm's per-segment (mean, M2, count) partials instead of a second read-only pass over the joined tensor.
// ACC (round 5): the branch's InstanceNorm arrives as accumulators (Affine::acc1, fav_internal.h) -- every block forms scale / shift
// for all C channels in its prologue (the arithmetic of in_finalize_kernel on exact integer sums) and keeps them in LDS; the launch
// uses at most 1024 blocks then (32 KB of accumulator words per block)
template <bool ACC>
__global__ __launch_bounds__(256) void res_add_kernel(const float* y, const float* scale, const float* shift,
                                                      const float* skip, int SW, int shave, const Affine sa,
                                                      int OH, int OW, int C, float* z, const Affine br)
{
    __shared__ float ss[ACC ? 2048 : 4];       // [scale C | shift C], C <= 1024
    if (ACC) {
        for (int i = threadIdx.x; i < C; i += 256) {
            long long w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
            for (int cp = 0; cp < STAT_COPIES; ++cp) {
                const longlong2* a = reinterpret_cast<const longlong2*>(br.acc1 + ((size_t)cp * C + i) * 4);
                const longlong2 lo = a[0], hi = a[1];
                w0 += lo.x; w1 += lo.y; w2 += hi.x; w3 += hi.y;
            }
            const double s1 = ((double)w1 * 4294967296.0 + (double)w0) * (1.0 / 1099511627776.0);
            const double s2 = ((double)w3 * 4294967296.0 + (double)w2) * (1.0 / 1099511627776.0);
            const double mean = s1 / (double)br.count1;
            double var = s2 / (double)br.count1 - mean * mean;
            var = var > 0.0 ? var : 0.0;
            const double sc = stat_acc_poisoned(w1, w3) ? (double)NAN : (double)br.gamma1[i] / sqrt(var + (double)br.eps1);
            ss[i] = (float)sc; ss[C + i] = (float)((double)br.beta1[i] - mean * sc);
            if (blockIdx.x == 0) {      // the other parity's accumulators: zero for the next frame
#pragma unroll
                for (int cp = 0; cp < STAT_COPIES; ++cp) {
                    longlong2* zz = reinterpret_cast<longlong2*>(br.acc1_zero + ((size_t)cp * C + i) * 4);
                    zz[0] = longlong2{0, 0}; zz[1] = longlong2{0, 0};
                }
            }
        }
        __syncthreads();
        scale = ss; shift = ss + C;
    }
    const int groups = C >> 2;
    const size_t total = (size_t)OH * OW * groups;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int g = (int)(idx % groups);
        const size_t pix = idx / groups;
        const int oy = (int)(pix / OW), ox = (int)(pix - (size_t)oy * OW);
        float4 v = *reinterpret_cast<const float4*>(y + pix * C + 4 * g);
        v = affine4(v, scale + 4 * g, shift + 4 * g, 0);
        float4 k = *reinterpret_cast<const float4*>(skip + ((size_t)(oy + shave) * SW + ox + shave) * C + 4 * g);
        k = apply_affine_g(k, sa, 4 * g);
        v.x += k.x; v.y += k.y; v.z += k.z; v.w += k.w;
        *reinterpret_cast<float4*>(z + pix * C + 4 * g) = v;
    }
}

template <int NPT>      // > 0: the joined values of the segment stay in registers for the M2 sweep (128 / (256 / (C / 4)) float4 per thread)
__global__ __launch_bounds__(256) void res_add_stats_kernel(const float* y, const float* scale, const float* shift,
                                                            const float* skip, int SW, int shave, const Affine sa,
                                                            int OW, int C, float* z, float2* partials, int* counts)
{
    __shared__ float red[1024];
    __shared__ float mean_s[1024];
    const int t = threadIdx.x;
    const int groups = C >> 2, nl = 256 / groups;         // float4 groups per pixel, pixel lanes
    const int g = t % groups, pl = t / groups;
    const int segs = (OW + 127) / 128;
    const int oy = blockIdx.x / segs, x0 = (blockIdx.x - oy * segs) * 128;
    const int cnt = min(128, OW - x0);
    const bool active = pl < nl;
    const float* yr = y + ((size_t)oy * OW + x0) * C + 4 * g;
    const float* kr = skip + ((size_t)(oy + shave) * SW + x0 + shave) * C + 4 * g;
    float* zr = z + ((size_t)oy * OW + x0) * C + 4 * g;
    float4 sm = make_float4(0, 0, 0, 0);
    float4 keep[NPT > 0 ? NPT : 1];
    if (NPT > 0) {
        float4 kk[NPT > 0 ? NPT : 1];
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int px = pl + i * nl;
            keep[i] = make_float4(0, 0, 0, 0); kk[i] = make_float4(0, 0, 0, 0);
            if (px < cnt) { keep[i] = *reinterpret_cast<const float4*>(yr + (size_t)px * C); kk[i] = *reinterpret_cast<const float4*>(kr + (size_t)px * C); }
        }
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int px = pl + i * nl;
            float4 v = affine4(keep[i], scale + 4 * g, shift + 4 * g, 0);
            const float4 k = apply_affine_g(kk[i], sa, 4 * g);
            v.x += k.x; v.y += k.y; v.z += k.z; v.w += k.w;
            if (px < cnt) { *reinterpret_cast<float4*>(zr + (size_t)px * C) = v; sm.x += v.x; sm.y += v.y; sm.z += v.z; sm.w += v.w; }
            keep[i] = v;
        }
    } else if (active)
        for (int px = pl; px < cnt; px += nl) {
            float4 v = *reinterpret_cast<const float4*>(yr + (size_t)px * C);
            v = affine4(v, scale + 4 * g, shift + 4 * g, 0);
            float4 k = *reinterpret_cast<const float4*>(kr + (size_t)px * C);
            k = apply_affine_g(k, sa, 4 * g);
            v.x += k.x; v.y += k.y; v.z += k.z; v.w += k.w;
            *reinterpret_cast<float4*>(zr + (size_t)px * C) = v;
            sm.x += v.x; sm.y += v.y; sm.z += v.z; sm.w += v.w;
        }
    if (active) *reinterpret_cast<float4*>(red + pl * C + 4 * g) = sm;
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        float r = 0;
        for (int i = 0; i < nl; ++i) r += red[i * C + c];
        mean_s[c] = r / (float)cnt;
    }
    __syncthreads();
    float4 q = make_float4(0, 0, 0, 0);
    if (active) {
        const float4 mu = *reinterpret_cast<const float4*>(mean_s + 4 * g);
        if (NPT > 0) {
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const float4 v = keep[i];
                const float dx = v.x - mu.x, dy = v.y - mu.y, dz = v.z - mu.z, dw = v.w - mu.w;
                if (pl + i * nl < cnt) { q.x = fmaf(dx, dx, q.x); q.y = fmaf(dy, dy, q.y); q.z = fmaf(dz, dz, q.z); q.w = fmaf(dw, dw, q.w); }
            }
        } else
        for (int px = pl; px < cnt; px += nl) {
            const float4 v = *reinterpret_cast<const float4*>(zr + (size_t)px * C);      // this thread's own stores
            const float dx = v.x - mu.x, dy = v.y - mu.y, dz = v.z - mu.z, dw = v.w - mu.w;
            q.x = fmaf(dx, dx, q.x); q.y = fmaf(dy, dy, q.y); q.z = fmaf(dz, dz, q.z); q.w = fmaf(dw, dw, q.w);
        }
        *reinterpret_cast<float4*>(red + pl * C + 4 * g) = q;
    }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        float r = 0;
        for (int i = 0; i < nl; ++i) r += red[i * C + c];
        partials[(size_t)blockIdx.x * C + c] = make_float2(mean_s[c], r);
    }
    if (t == 0) counts[blockIdx.x] = cnt;
}

__device__ __forceinline__ int reflect(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// NCHW -> reflection-padded NHWC with channel padding (nn.SpatialReflectionPadding, train_video.lua:319-325)
__global__ __launch_bounds__(256) void nchw_to_nhwc_pad_kernel(const float* in, int C, int H, int W, int pad, int Cp,
                                                               float* out)
{
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const size_t total = (size_t)Hp * Wp * Cp;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int c = (int)(idx % Cp);
        const size_t pix = idx / Cp;
        const int y = (int)(pix / Wp), x = (int)(pix - (size_t)y * Wp);
        float v = 0.f;
        if (c < C) v = in[((size_t)c * H + reflect(y - pad, H)) * W + reflect(x - pad, W)];
        out[idx] = v;
    }
}

__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* in, int M, int C, const Affine a, float* out)
{
    const size_t total = (size_t)M * C;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int c = (int)(idx / M);
        const size_t m = idx - (size_t)c * M;
        float v = in[m * C + c];
        if (a.stages >= 1) {
            v = fmaf(v, a.scale1[c], a.shift1[c]); if (a.relu1) v = fmaxf(v, 0.f);
            if (a.stages >= 2) { v = fmaf(v, a.scale2[c], a.shift2[c]); if (a.relu2) v = fmaxf(v, 0.f); }
        }
        out[idx] = v;
    }
}

inline int grid_for(size_t total) { size_t b = (total + 255) / 256; return (int)(b > 8192 ? 8192 : (b ? b : 1)); }

}  // namespace

int launch_in_finalize(const float* partials, const int* counts, int mblocks, int M, int block_pixels, int C, int Cpitch,
                       const float* gamma, const float* beta, float eps, float* scale, float* shift, hipStream_t st)
{
    hipLaunchKernelGGL(in_finalize_kernel, dim3(C), dim3(256), 0, st, reinterpret_cast<const float2*>(partials), counts,
                       mblocks, M, block_pixels, Cpitch, gamma, beta, eps, scale, shift);
    FAV_LAUNCH_CHECK("in_finalize_kernel");
    return FAV_OK;
}

int launch_stats(const float* x, int M, int C, const Affine& t, float* partials, hipStream_t st)
{
    FAV_REQUIRE(C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0, "stats: unsupported channel count %d", C);
    const dim3 grid((M + 127) / 128);
    float2* pp = reinterpret_cast<float2*>(partials);
    if (C == 64) hipLaunchKernelGGL(stats_kernel<8>, grid, dim3(256), 0, st, x, M, C, t, pp);
    else if (C == 128) hipLaunchKernelGGL(stats_kernel<16>, grid, dim3(256), 0, st, x, M, C, t, pp);
    else hipLaunchKernelGGL(stats_kernel<0>, grid, dim3(256), 0, st, x, M, C, t, pp);
    FAV_LAUNCH_CHECK("stats_kernel");
    return FAV_OK;
}

int launch_res_add(const float* y, const float* scale, const float* shift, const float* skip, int SH, int SW,
                   int shave, const Affine& skip_t, int C, float* z, float* partials, int* counts, hipStream_t st, int skip_pitch, const Affine* branch_acc)
{
    const int OH = SH - 2 * shave, OW = SW - 2 * shave;
    if (skip_pitch > 0) SW = skip_pitch;              // the kernels use SW as the skip's row pitch only
    FAV_REQUIRE(C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0 && OH > 0 && OW > 0, "res_add: bad shape (C=%d)", C);
    FAV_REQUIRE(!(partials && branch_acc && branch_acc->acc1), "res_add: the statistics-taking join does not take an accumulator-form InstanceNorm");
    if (partials) {
        const dim3 grid(res_add_stat_blocks(OH, OW));
        float2* pp = reinterpret_cast<float2*>(partials);
        if (C == 128) hipLaunchKernelGGL(res_add_stats_kernel<16>, grid, dim3(256), 0, st, y, scale, shift, skip, SW, shave, skip_t, OW, C, z, pp, counts);
        else if (C == 64) hipLaunchKernelGGL(res_add_stats_kernel<8>, grid, dim3(256), 0, st, y, scale, shift, skip, SW, shave, skip_t, OW, C, z, pp, counts);
        else hipLaunchKernelGGL(res_add_stats_kernel<0>, grid, dim3(256), 0, st, y, scale, shift, skip, SW, shave, skip_t, OW, C, z, pp, counts);
    }
    else if (branch_acc != nullptr && branch_acc->acc1 != nullptr)
        hipLaunchKernelGGL(res_add_kernel<true>, dim3(std::min(1024, grid_for((size_t)OH * OW * (C / 4)))), dim3(256), 0, st, y, scale, shift, skip, SW, shave, skip_t,
                           OH, OW, C, z, *branch_acc);
    else
        hipLaunchKernelGGL(res_add_kernel<false>, dim3(grid_for((size_t)OH * OW * (C / 4))), dim3(256), 0, st, y, scale, shift, skip, SW, shave, skip_t,
                           OH, OW, C, z, Affine());
    FAV_LAUNCH_CHECK("res_add_kernel");
    return FAV_OK;
}

int launch_nchw_to_nhwc_pad(const float* in, int C, int H, int W, int pad, int Cp, float* out, hipStream_t st)
{
    FAV_REQUIRE(pad < H && pad < W, "reflection pad %d must be smaller than the image (%dx%d)", pad, W, H);
    hipLaunchKernelGGL(nchw_to_nhwc_pad_kernel, dim3(grid_for((size_t)(H + 2 * pad) * (W + 2 * pad) * Cp)), dim3(256), 0,
                       st, in, C, H, W, pad, Cp, out);
    FAV_LAUNCH_CHECK("nchw_to_nhwc_pad_kernel");
    return FAV_OK;
}

int launch_nhwc_to_nchw(const float* in, int M, int C, const Affine& t, float* out, hipStream_t st)
{
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for((size_t)M * C)), dim3(256), 0, st, in, M, C, t, out);
    FAV_LAUNCH_CHECK("nhwc_to_nchw_kernel");
    return FAV_OK;
}

}  // namespace fav
