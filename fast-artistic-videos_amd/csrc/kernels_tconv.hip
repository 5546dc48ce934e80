// kernels_tconv.hip -- nn.SpatialFullConvolution (`u<n>`: 3x3 stride 2, and every `f<k>s<s>-<n>` of models_video.lua:81-89,99-102) computed
// by OUTPUT PHASE on the physical input (tconv_pack.h): each of the s x s phases (oy mod s, ox mod s) is a small stride-1 correlation,
// k^2 / s^2 multiplies per output -- 2.25 for `u<n>` instead of the 9 that the zero-stuffed form on the generic kernel executes.
//
// Unit of work = a tile of 8 x 32 input pixels (u coordinates: output pixel o = s u + c) plus its halo [lo, hi] (tconv_pack.h):
//   * block = 4 waves (two blocks per CU: 189 registers, no scratch); wave = one ITEM (phase, tile of 32 output channels) of the tile: 8 accumulators (one per tile row, 32 pixels x 32
//     channels each).  blockIdx.y counts the groups of four items: the four phases of a stride-2 layer's 32 filters are one block
//   * input: per slice of 32 channels the (8 + hi - lo) x (32 + hi - lo) halo is staged in LDS once (pixel pitch 36 floats), with the
//     producer's pending InstanceNorm / BatchNorm (+ ReLU) applied on the way; pixels outside the image are zero AFTER that transform
//   * a wave's taps are the halo shifted by its phase's offsets; weights come in the packed order (fragment order, one 1 KiB load per
//     32 MFMAs, requested one tap ahead) global -> registers
//   * epilogue: bias, NHWC stores to (s u + c), and the (mean, M2) partial of the item's pixels: statistics entry tile * s^2 + phase,
//     counts[entry] = its valid pixels (the same for every channel tile) -- no merge between waves
// A plain data-parallel grid: blocks share nothing and wait for nobody.
#include <algorithm>

#include "fav_internal.h"
#include "conv_device.h"
#include "launch_common.h"
#include "tconv_pack.h"

namespace fav {

namespace {

struct TconvArgs {
    const float* in; const float* wpk; const float* bias;
    const float* scale1; const float* shift1; const float* scale2; const float* shift2;
    float* out; float2* partials; int* counts;
    int IH, IW, IWp, CIN, COUT, COUTp, OH, OW;
    int k, s, p, lo, HH, HW, hw_magic;      // halo rows / columns; pix / HW = (pix * hw_magic) >> 20 for pix < 1024
    int tiles_x, nitems, stages, relu1, relu2;
};

__global__ __launch_bounds__(256, 2) void conv_tconv_kernel(const TconvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float Hs[];      // [HH * HW][LDSS]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int m = lane & 31, h = lane >> 5;
    const int k = a.k, s = a.s, p = a.p, kk = k * k, nph = s * s, HW = a.HW;
    const int tile = blockIdx.x, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int uy0 = ty * TCONV_TILE_H, ux0 = tx * TCONV_TILE_W;

    // this wave's item: phase (cy, cx) of the channel tile nt
    const int item = blockIdx.y * 4 + wave;
    const bool active = item < a.nitems;
    const int nt = active ? item / nph : 0, ph = active ? item - nt * nph : 0;
    const int cy = ph / s, cx = ph - cy * s;
    const int nty = tconv_ntap(k, s, p, cy), ntx = tconv_ntap(k, s, p, cx);
    const int T = active ? nty * ntx : 0;
    const int slot0 = tconv_slot0(k, s, p, cy, cx);
    const int nkg = a.CIN >> 3, nslices = (nkg + 3) >> 2;
    const float* const wl = a.wpk + (size_t)nt * nkg * kk * 256 + lane * 4;      // + (kg * kk + slot0 + tap) * 256
    // fragments: tile row j, tap (jy, jx), channel group kg -> halo pixel (j + dy - lo - jy, m + dx - lo - jx), channels kg * 8 + 4 h ..
    const float* const ab = Hs + ((tconv_tap_off(s, p, cy, 0) - a.lo) * HW + tconv_tap_off(s, p, cx, 0) - a.lo + m) * LDSS + 4 * h;

    f32x16 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int npx = a.HH * HW, q = t & 7;
    v4f bn = {0.f, 0.f, 0.f, 0.f};
    if (T > 0) bn = *reinterpret_cast<const v4f*>(wl + (size_t)slot0 * 256);
    int nkgg = 0, ntp = 0;                  // the (channel group, tap) whose weights are in bn

    for (int sl = 0; sl < nslices; ++sl) {
        // ---- stage the slice: thread = (pixel t >> 3 + 32 i, 16-byte chunk q)
        const int c0 = sl * 32 + q * 4;
        const bool qok = c0 < a.CIN;
        v4f sc1 = {1.f, 1.f, 1.f, 1.f}, sh1 = {0.f, 0.f, 0.f, 0.f}, sc2 = sc1, sh2 = sh1;
        if (qok && a.stages >= 1) { sc1 = *reinterpret_cast<const v4f*>(a.scale1 + c0); sh1 = *reinterpret_cast<const v4f*>(a.shift1 + c0); }
        if (qok && a.stages >= 2) { sc2 = *reinterpret_cast<const v4f*>(a.scale2 + c0); sh2 = *reinterpret_cast<const v4f*>(a.shift2 + c0); }
        const float lo1 = (a.stages >= 1 && a.relu1) ? 0.f : -INFINITY, lo2 = (a.stages >= 2 && a.relu2) ? 0.f : -INFINITY;
        __syncthreads();                    // the previous slice's fragments have been read
#pragma unroll 4
        for (int pix = t >> 3; pix < npx; pix += 32) {
            const int hy = (pix * a.hw_magic) >> 20, hx = pix - hy * HW;
            const int iy = uy0 + a.lo + hy, ix = ux0 + a.lo + hx;
            v4f v = {0.f, 0.f, 0.f, 0.f};
            if (qok && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW) {
                v = *reinterpret_cast<const v4f*>(a.in + ((size_t)iy * a.IWp + ix) * a.CIN + c0);
                if (a.stages >= 1) {
                    v.x = fmaxf(fmaf(v.x, sc1.x, sh1.x), lo1); v.y = fmaxf(fmaf(v.y, sc1.y, sh1.y), lo1);
                    v.z = fmaxf(fmaf(v.z, sc1.z, sh1.z), lo1); v.w = fmaxf(fmaf(v.w, sc1.w, sh1.w), lo1);
                }
                if (a.stages >= 2) {
                    v.x = fmaxf(fmaf(v.x, sc2.x, sh2.x), lo2); v.y = fmaxf(fmaf(v.y, sc2.y, sh2.y), lo2);
                    v.z = fmaxf(fmaf(v.z, sc2.z, sh2.z), lo2); v.w = fmaxf(fmaf(v.w, sc2.w, sh2.w), lo2);
                }
            }
            *reinterpret_cast<v4f*>(Hs + pix * LDSS + q * 4) = v;
        }
        __syncthreads();

        // ---- this slice's channel groups x the phase's taps: 32 MFMAs per (group, tap)
        if (T > 0) {
            const int nkgs = min(4, nkg - sl * 4);
            for (int kg = 0; kg < nkgs; ++kg)
                for (int jy = 0; jy < nty; ++jy)
                    for (int jx = 0; jx < ntx; ++jx) {
                        const v4f b = bn;
                        // the next tap's weights (the last one asks for itself again)
                        if (++ntp == T) { ntp = 0; ++nkgg; }
                        if (nkgg == nkg) { nkgg = nkg - 1; ntp = T - 1; }
                        bn = *reinterpret_cast<const v4f*>(wl + ((size_t)nkgg * kk + slot0 + ntp) * 256);
                        const float* const ap = ab + kg * 8 - (jy * HW + jx) * LDSS;
#pragma unroll
                        for (int hf = 0; hf < 2; ++hf) {
                            v4f fa[4];
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) fa[jj] = *reinterpret_cast<const v4f*>(ap + (4 * hf + jj) * HW * LDSS);
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) acc[4 * hf + jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[jj].x, b.x, acc[4 * hf + jj], 0, 0, 0);
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) acc[4 * hf + jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[jj].y, b.y, acc[4 * hf + jj], 0, 0, 0);
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) acc[4 * hf + jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[jj].z, b.z, acc[4 * hf + jj], 0, 0, 0);
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) acc[4 * hf + jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[jj].w, b.w, acc[4 * hf + jj], 0, 0, 0);
                        }
                    }
        }
    }
    if (!active) return;                    // (no barrier below)

    // ---- epilogue: acc[j][r] = output (s (uy0 + j) + cy, s (ux0 + mi) + cx), channel nt * 32 + n;  mi = (r & 3) + 8 (r >> 2) + 4 h
    const int n = lane & 31, co = nt * 32 + n;
    const float bv = a.bias[co];
    const bool cok = co < a.COUT;
    float sm = 0.f; int nv = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int oy = s * (uy0 + j) + cy;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ox = s * (ux0 + (r & 3) + 8 * (r >> 2) + 4 * h) + cx;
            const float v = acc[j][r] + bv;
            acc[j][r] = v;
            if (oy < a.OH && ox < a.OW) {
                if (cok) a.out[((size_t)oy * a.OW + ox) * a.COUT + co] = v;
                sm += v; ++nv;
            }
        }
    }
    if (a.partials != nullptr) {
        const int nw = nv + __shfl_xor(nv, 32);
        const float ssum = sm + __shfl_xor(sm, 32);
        const float mu = nw ? ssum / (float)nw : 0.f;
        float qq = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int oy = s * (uy0 + j) + cy;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ox = s * (ux0 + (r & 3) + 8 * (r >> 2) + 4 * h) + cx;
                const float d = acc[j][r] - mu;
                if (oy < a.OH && ox < a.OW) qq = fmaf(d, d, qq);
            }
        }
        qq += __shfl_xor(qq, 32);
        const size_t entry = (size_t)tile * nph + ph;
        if (lane < 32) a.partials[entry * a.COUTp + co] = make_float2(mu, qq);
        if (lane == 0 && nt == 0) a.counts[entry] = nw;
    }
}

}  // namespace

bool conv_tconv_eligible(const ConvShape& s)
{
    return s.transposed && s.cin_pitch % 8 == 0 && s.cin_pitch >= 8 && s.coutp % 32 == 0 && s.coutp >= 32 && s.k >= 1 && s.k <= TCONV_MAX_K &&
           s.stride >= 2 && s.stride <= TCONV_MAX_S && s.pad >= 0 && s.pad <= s.k - 1 && s.adj >= 0 && s.adj < s.stride && s.ups == 0;
}
int conv_tconv_tiles(const ConvLaunch& c)
{
    const int UH = (c.OH + c.stride - 1) / c.stride, UW = (c.OW + c.stride - 1) / c.stride;
    return ((UH + TCONV_TILE_H - 1) / TCONV_TILE_H) * ((UW + TCONV_TILE_W - 1) / TCONV_TILE_W) * c.stride * c.stride;
}

// c: the PHYSICAL input (IH x IW, ups 0), KH = k, stride / pad as the module has them, OH x OW = (in - 1) s - 2 p + k + adj
int launch_conv_tconv(const ConvLaunch& c, hipStream_t st)
{
    const int k = c.KH, s = c.stride, p = c.pad;
    FAV_REQUIRE(c.KH == c.KW && c.wpk && !c.final_mode && !c.stuff && c.OWp == 0 && c.pre.acc1 == nullptr && c.pre.stages <= 2 && c.join_skip == nullptr,
                "transposed conv: not eligible");
    const int adj = c.OH - ((c.IH - 1) * s - 2 * p + k);
    FAV_REQUIRE(conv_tconv_eligible(conv_shape(c, 1, adj)) && c.COUT <= c.COUTp && c.IH > 0 && c.IW > 0 &&
                c.OW == (c.IW - 1) * s - 2 * p + k + adj && c.OH > 0 && c.OW > 0 && c.IWp >= c.IW, "transposed conv: bad geometry");
    FAV_REQUIRE(c.partials == nullptr || c.counts != nullptr, "transposed conv: statistics without counts");
    TconvArgs a;
    a.in = c.in; a.wpk = c.wpk; a.bias = c.bias;
    a.scale1 = c.pre.scale1; a.shift1 = c.pre.shift1; a.scale2 = c.pre.scale2; a.shift2 = c.pre.shift2;
    a.stages = c.pre.stages; a.relu1 = c.pre.relu1; a.relu2 = c.pre.relu2;
    a.out = c.out; a.partials = reinterpret_cast<float2*>(c.partials); a.counts = c.counts;
    a.IH = c.IH; a.IW = c.IW; a.IWp = c.IWp; a.CIN = c.CIN; a.COUT = c.COUT; a.COUTp = c.COUTp; a.OH = c.OH; a.OW = c.OW;
    a.k = k; a.s = s; a.p = p; a.lo = tconv_lo(k, s, p);
    const int span = tconv_hi(k, s, p) - a.lo;
    a.HH = TCONV_TILE_H + span; a.HW = TCONV_TILE_W + span; a.hw_magic = (1 << 20) / a.HW + 1;
    const int UH = (c.OH + s - 1) / s, UW = (c.OW + s - 1) / s;
    a.tiles_x = (UW + TCONV_TILE_W - 1) / TCONV_TILE_W;
    const int tiles = a.tiles_x * ((UH + TCONV_TILE_H - 1) / TCONV_TILE_H);
    a.nitems = s * s * (c.COUTp / 32);
    const size_t lds = (size_t)a.HH * a.HW * LDSS * sizeof(float);
    FAV_REQUIRE(a.HH * a.HW < 1024 && a.HW <= 64 && lds <= 160 * 1024, "transposed conv: halo too large");
    FAV_REQUIRE(tiles <= 0x7fffffff / (s * s) && (a.nitems + 3) / 4 <= 65535, "transposed conv: grid too large");
    static PerDevice cache; int cus;
    FAV_HIP(launch_cus(cache, &cus, conv_tconv_kernel));
    hipLaunchKernelGGL(conv_tconv_kernel, dim3(tiles, (a.nitems + 3) / 4), dim3(256), lds, st, a);
    FAV_LAUNCH_CHECK("conv_tconv_kernel");
    return FAV_OK;
}

}  // namespace fav
