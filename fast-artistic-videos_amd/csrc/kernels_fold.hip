// kernels_fold.hip -- the two row-folded last-layer kernels (conv_rowfold_kernel, conv_rowfold_up2_kernel).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "fav_internal.h"
#include "conv_device.h"
#include "launch_common.h"

namespace fav {

// ------------------------------------------------------------------------------------------------
// Last layer (c9s1-3: 64 -> 3 channels, 9x9): "row-folded" implicit GEMM.
// With only 3 output channels a pixels x channels GEMM would waste 29/32 of every MFMA.  Instead the
// kx taps are folded into the N dimension: for one output row y
//     D[x'][(c,kx)] = sum_{ky,ci} in[y+ky-p][x'][ci] * w[c][ci][ky][kx]        (M = 128 input columns x',
//                                                                               N = 3*9 = 27 -> 32,
//                                                                               K = 9*64 = 576)
//     out[y][x][c]  = sum_kx D[x+kx-p][(c,kx)]                                  (diagonal sum, done in LDS)
// MFMA utilisation = 27/32 * 120/128 = 79 % instead of 9 %.  A block (8 waves: 4 column groups x 2 row halves)
// owns R = 8 output rows x 120 output columns: every staged (transformed, nearest-upsampled) input row feeds up to 8 output rows with 8
// different ky weight slices, all 9 slices stay resident in LDS, and with x2 upsampling each physical
// input row is staged once for its two logical rows.  Epilogue: bias, Tanh, MulConstant, VGG de-process.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int FOLD_R = 16;       // output rows per tile
constexpr int FOLD_M = 128;      // input columns per tile

struct FoldArgs {
    const float* in; const float* wfold; const float* bias;
    const float* scale1; const float* shift1; const float* scale2; const float* shift2;
    float* out_planar; float* out_raw;
    int IH, IW, IWp, ups, COUT, KH, KW, pad, OH, OW;
    int stages, relu1, relu2;
    float tanh_mul;
    int tiles_x, tiles_y;
    long long* dbg;      // optional in-kernel timeline (FAV_FOLD_DBG): per block tile count and the time spent in staging+MFMA loop / epilogue
};

// 16 output rows per tile (8 accumulators per wave): every staged input row feeds up to 9 output rows, so a taller tile stages
// (16 + 8) / 16 = 1.5 input rows per output row instead of 2, and the per-tile costs (the first row's latency, the ramp of
// half-used rows at the top and bottom, the diagonal-sum epilogue) are paid 495 instead of 990 times per 1280x720 frame.
// Persistent blocks: the nine ky weight slices (78 KB) are loaded into LDS once per block, not once per tile.
template <int CIN>
__global__ __launch_bounds__(512, 2) void conv_rowfold_kernel(const FoldArgs p)
{
    constexpr int NT = 512;                    // 8 waves: waves 0-3 own output rows 0-7, waves 4-7 rows 8-15 (same columns)
    constexpr int RW = FOLD_R / 2;             // output rows per wave
    constexpr int S = CIN + 4;                 // LDS row stride (floats): odd multiple of 16 B -> conflict-free b128
    constexpr int NV = CIN / 16;               // float4 per thread per staged row (4 threads per column)
    constexpr int KK = CIN / 8;                // fragment steps per row (8 k values each)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Bs = smem;                          // [KH][32][S]
    float* aff = Bs + p.KH * 32 * S;           // [4][CIN]
    float* As = aff + 4 * CIN;                 // [2][FOLD_M][S]; the epilogue's D tile reuses it

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wcol = wave & 3, wrow = wave >> 2;
    const int XO = FOLD_M - (p.KW - 1);        // output columns per tile

    for (int i = t; i < CIN; i += NT) {
        aff[i] = p.stages >= 1 ? p.scale1[i] : 1.f; aff[CIN + i] = p.stages >= 1 ? p.shift1[i] : 0.f;
        aff[2 * CIN + i] = p.stages >= 2 ? p.scale2[i] : 1.f; aff[3 * CIN + i] = p.stages >= 2 ? p.shift2[i] : 0.f;
    }
    const float lo1 = (p.stages >= 1 && p.relu1) ? 0.f : -INFINITY;
    const float lo2 = (p.stages >= 2 && p.relu2) ? 0.f : -INFINITY;
    // all ky weight slices -> LDS, once per block (wfold is [KH][32][CIN], zero rows for n >= COUT*KW)
    for (int e = t; e < p.KH * 32 * (CIN / 4); e += NT) {
        const int row = e / (CIN / 4), c4 = e - row * (CIN / 4);
        *reinterpret_cast<v4f*>(Bs + row * S + c4 * 4) = *reinterpret_cast<const v4f*>(p.wfold + (size_t)row * CIN + c4 * 4);
    }
    // staging assignment: column xl = t>>2 of the tile, channel quarter (t&3)
    const int xl = t >> 2, ch0 = (t & 3) * (CIN / 4);
    const int frag = (lane & 31) * S + (lane >> 5) * 4;
    const int col = lane & 31, rbase = 4 * (lane >> 5);
    float4 ra[NV];

    for (int tile = blockIdx.x; tile < p.tiles_x * p.tiles_y; tile += gridDim.x) {
        const int by = tile / p.tiles_x, bx = tile - by * p.tiles_x;
        const int ox0 = bx * XO, oy0 = by * FOLD_R;
        const int xs = ox0 - p.pad;                // first input column of the tile (may be negative)
        const int iy_lo = max(0, oy0 - p.pad), iy_hi = min(p.IH - 1, oy0 + FOLD_R - 1 + p.KH - 1 - p.pad);
        const int pr_lo = iy_lo >> p.ups, pr_hi = iy_hi >> p.ups;
        const int ix = xs + xl;
        const bool colv = ix >= 0 && ix < p.IW;
        const float colm = colv ? 1.f : 0.f;
        const int coloff = colv ? (ix >> p.ups) * CIN + ch0 : 0;

#define FOLD_LOAD(pr_)                                                                              \
        {                                                                                           \
            const float* src_ = p.in + (size_t)(pr_) * p.IWp * CIN + coloff;                        \
            _Pragma("unroll") for (int i = 0; i < NV; ++i) ra[i] = *reinterpret_cast<const float4*>(src_ + 4 * i); \
        }
#define FOLD_STORE(buf_)                                                                            \
        {                                                                                           \
            float* dst_ = As + (buf_) * FOLD_M * S + xl * S + ch0;                                  \
            _Pragma("unroll") for (int i = 0; i < NV; ++i) {                                        \
                float4 v_ = affine4_lo(ra[i], aff + ch0 + 4 * i, aff + CIN + ch0 + 4 * i, lo1);     \
                v_ = affine4_lo(v_, aff + 2 * CIN + ch0 + 4 * i, aff + 3 * CIN + ch0 + 4 * i, lo2); \
                v_.x *= colm; v_.y *= colm; v_.z *= colm; v_.w *= colm;                             \
                *reinterpret_cast<float4*>(dst_ + 4 * i) = v_;                                      \
            }                                                                                       \
        }

        f32x16 acc[RW];
#pragma unroll
        for (int y = 0; y < RW; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[y][r] = 0.f;

        FOLD_LOAD(pr_lo);
        __syncthreads();               // affine tables + weights visible; the previous tile's epilogue is done with the staging memory
        FOLD_STORE(0);
        __syncthreads();

        int cur = 0;
        for (int pr = pr_lo; pr <= pr_hi; ++pr) {
            const bool more = pr < pr_hi;
            if (more) FOLD_LOAD(pr + 1);
            const float* a_base = As + cur * FOLD_M * S + wcol * 32 * S + frag;
            const int iy_first = max(iy_lo, pr << p.ups), iy_last = min(iy_hi, ((pr + 1) << p.ups) - 1);
            for (int iy = iy_first; iy <= iy_last; ++iy) {
                const int kyb = iy - oy0 + p.pad - wrow * RW;      // ky for this wave's output row yy is kyb - yy
                // the row's A fragments are read once and serve every output row it feeds; per output row one wave-uniform test,
                // then a straight-line block of KK weight-fragment reads and 4 KK MFMAs (LDS latency hides inside it)
                float4 af[KK];
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) af[kk] = *reinterpret_cast<const float4*>(a_base + kk * 8);
#pragma unroll
                for (int yy = 0; yy < RW; ++yy) {
                    const int ky = kyb - yy;
                    if (ky >= 0 && ky < p.KH) {            // wave-uniform
                        const float* b_base = Bs + ky * 32 * S + frag;
#pragma unroll
                        for (int kk = 0; kk < KK; ++kk) {
                            const float4 bf = *reinterpret_cast<const float4*>(b_base + kk * 8);
                            acc[yy] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].x, bf.x, acc[yy], 0, 0, 0);
                            acc[yy] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].y, bf.y, acc[yy], 0, 0, 0);
                            acc[yy] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].z, bf.z, acc[yy], 0, 0, 0);
                            acc[yy] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].w, bf.w, acc[yy], 0, 0, 0);
                        }
                    }
                }
            }
            if (more) FOLD_STORE(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
#undef FOLD_LOAD
#undef FOLD_STORE

        // ---- epilogue in four passes of 4 output rows (2 of each row half): D tiles -> LDS [4][128][33] in the staging area (the
        // weights stay resident), then the diagonal sum over kx
        float* D = As;
        const size_t MO = (size_t)p.OH * p.OW;
        const int per_row = XO * p.COUT;
        constexpr int PR = 2;              // rows of each half per pass
#pragma unroll
        for (int h = 0; h < RW / PR; ++h) {
#pragma unroll
            for (int y2 = 0; y2 < PR; ++y2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int xr = wcol * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                    D[((wrow * PR + y2) * FOLD_M + xr) * 33 + col] = acc[h * PR + y2][r];
                }
            __syncthreads();
            for (int e = t; e < 2 * PR * per_row; e += NT) {
                const int yl = e / per_row, rem = e - yl * per_row;            // D row: half = yl / PR, y2 = yl % PR
                const int c = rem / XO, xo = rem - c * XO;
                const int oy = oy0 + (yl / PR) * RW + h * PR + (yl % PR), ox = ox0 + xo;
                if (oy >= p.OH || ox >= p.OW) continue;
                float v = p.bias[c];
                const float* d = D + (yl * FOLD_M + xo) * 33 + c * p.KW;
                for (int kx = 0; kx < p.KW; ++kx) v += d[kx * 33 + kx];
                v = tanhf(v) * p.tanh_mul;                                              // models_video.lua:135-136
                const size_t o = (size_t)oy * p.OW + ox;
                if (p.out_raw) p.out_raw[(size_t)c * MO + o] = v;
                if (p.out_planar) {
                    const float mean = c == 0 ? 103.939f : (c == 1 ? 116.779f : 123.68f);
                    p.out_planar[(size_t)(2 - c) * MO + o] = (v + mean) / 255.f;          // preprocess.lua:66-71
                }
            }
            __syncthreads();
        }
    }
}

// The same layer when its input is a x2 nearest-upsampled tensor (U2 before c9s1-3, models_video.lua:129-133): the upsampled
// image holds every physical pixel four times, so three quarters of the products above are repeats.
//   * columns: D[x'][(c,kx)] is identical for the logical columns 2v and 2v+1 -- it is computed once per PHYSICAL column and the
//     diagonal sum reads it at (x + kx - p) >> 1: half the GEMM rows, no change to the weights;
//   * rows: the logical input rows 2r and 2r+1 are the same data and reach output row y through ky0 = 2r - y + p and ky0 + 1, so the
//     physical row is multiplied ONCE by the merged slice  Wm[ky0 + 1] = W[ky0] + W[ky0 + 1]  (W[-1] = W[KH] = 0; KH + 1 merged
//     slices, summed on the host in double): five merged slices per output row instead of nine.
// 3.6x fewer MFMAs than on the upsampled image, same operands otherwise (the merged weights are the only re-association).
// Tile = 16 output rows x 120 output columns = 64 physical input columns: waves = 2 column groups x 4 row groups, a row group
// owning the output rows g, g+4, g+8, g+12 -- a physical row feeds ten CONSECUTIVE output rows, so the interleave gives every
// wave two or three 32-MFMA blocks per staged row (consecutive rows per wave would leave half the waves idle at each barrier).
constexpr int FOLD2_M = 64;      // physical input columns per tile

// NH > 1 (input pitch CT = NH * CIN channels, e.g. 128 behind a c3s1-128 of a checkpoint with more filters): the merged slices of all
// channels do not fit the LDS next to the staging buffers, so a tile is computed in NH passes over its rows, one per block of CIN
// channels, into the same accumulators; the pass's slices (87 KB for CIN = 64) are reloaded from L2 at its start -- ~1 us against the
// ~50 us a pass takes
template <int CIN, int NH = 1>
__global__ __launch_bounds__(512, 2) void conv_rowfold_up2_kernel(const FoldArgs p)
{
    constexpr int NT = 512;
    constexpr int CT = CIN * NH;               // channel pitch of the input tensor
    constexpr int RW = FOLD_R / 4;             // output rows per wave (rows g + 4 yy)
    constexpr int S = CIN + 4;
    constexpr int NV = CIN / 32;               // float4 per thread per staged row (8 threads per column)
    constexpr int KK = CIN / 8;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Bs = smem;                          // [KH + 1][32][S] merged slices
    float* aff = Bs + (p.KH + 1) * 32 * S;     // [4][CIN]
    float* As = aff + 4 * CIN;                 // [2][FOLD2_M][S]; the epilogue's D tile [4][FOLD2_M][33] reuses it

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wcol = wave & 1, wrow = wave >> 1;
    const int XO = 2 * FOLD2_M - (p.KW - 1);   // output columns per tile (120)
    const int PH = p.IH >> 1, PW = p.IW >> 1;  // physical input size

    const float lo1 = (p.stages >= 1 && p.relu1) ? 0.f : -INFINITY;
    const float lo2 = (p.stages >= 2 && p.relu2) ? 0.f : -INFINITY;
    const float* wm = p.wfold + (size_t)p.KH * 32 * CT;            // merged slices follow the plain ones
    // the transform table and the merged slices of channels hoff .. hoff + CIN - 1 (NH == 1: once per block; else once per pass)
#define FOLD_RESIDENT(hoff_)                                                                        \
    {                                                                                               \
        for (int i = t; i < CIN; i += NT) {                                                         \
            aff[i] = p.stages >= 1 ? p.scale1[(hoff_) + i] : 1.f; aff[CIN + i] = p.stages >= 1 ? p.shift1[(hoff_) + i] : 0.f; \
            aff[2 * CIN + i] = p.stages >= 2 ? p.scale2[(hoff_) + i] : 1.f; aff[3 * CIN + i] = p.stages >= 2 ? p.shift2[(hoff_) + i] : 0.f; \
        }                                                                                           \
        for (int e = t; e < (p.KH + 1) * 32 * (CIN / 4); e += NT) {                                 \
            const int row = e / (CIN / 4), c4 = e - row * (CIN / 4);                                \
            *reinterpret_cast<v4f*>(Bs + row * S + c4 * 4) = *reinterpret_cast<const v4f*>(wm + (size_t)row * CT + (hoff_) + c4 * 4); \
        }                                                                                           \
    }
    if (NH == 1) FOLD_RESIDENT(0);
    const int xl = t >> 3, ch0 = (t & 7) * (CIN / 8);
    const int frag = (lane & 31) * S + (lane >> 5) * 4;
    const int col = lane & 31, rbase = 4 * (lane >> 5);
    float4 ra[NV];

    for (int tile = blockIdx.x; tile < p.tiles_x * p.tiles_y; tile += gridDim.x) {
        const int by = tile / p.tiles_x, bx = tile - by * p.tiles_x;
        const int ox0 = bx * XO, oy0 = by * FOLD_R;
        const int pxs = (ox0 - p.pad) >> 1;        // first physical column of the tile (ox0 - pad is even; may be negative)
        const int iy_lo = max(0, oy0 - p.pad), iy_hi = min(p.IH - 1, oy0 + FOLD_R - 1 + p.KH - 1 - p.pad);
        const int pr_lo = iy_lo >> 1, pr_hi = min(iy_hi >> 1, PH - 1);
        const int pc = pxs + xl;
        const bool colv = pc >= 0 && pc < PW;
        const float colm = colv ? 1.f : 0.f;
        const int coloff = colv ? pc * CT + ch0 : 0;
        int hoff = 0;                              // first channel of the current pass

#define FOLD_LOAD(pr_)                                                                              \
        {                                                                                           \
            const float* src_ = p.in + (size_t)(pr_) * p.IWp * CT + coloff + hoff;                  \
            _Pragma("unroll") for (int i = 0; i < NV; ++i) ra[i] = *reinterpret_cast<const float4*>(src_ + 4 * i); \
        }
#define FOLD_STORE(buf_)                                                                            \
        {                                                                                           \
            float* dst_ = As + (buf_) * FOLD2_M * S + xl * S + ch0;                                 \
            _Pragma("unroll") for (int i = 0; i < NV; ++i) {                                        \
                float4 v_ = affine4_lo(ra[i], aff + ch0 + 4 * i, aff + CIN + ch0 + 4 * i, lo1);     \
                v_ = affine4_lo(v_, aff + 2 * CIN + ch0 + 4 * i, aff + 3 * CIN + ch0 + 4 * i, lo2); \
                v_.x *= colm; v_.y *= colm; v_.z *= colm; v_.w *= colm;                             \
                *reinterpret_cast<float4*>(dst_ + 4 * i) = v_;                                      \
            }                                                                                       \
        }

        f32x16 acc[RW];
#pragma unroll
        for (int y = 0; y < RW; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[y][r] = 0.f;

        const long long w0 = p.dbg ? wall_clock64() : 0;
        long long w1 = 0;
#pragma unroll 1
        for (int half = 0; half < NH; ++half) {
        hoff = half * CIN;
        FOLD_LOAD(pr_lo);
        __syncthreads();               // affine tables + weights visible; the previous tile's epilogue (the previous pass's last row) is done with the LDS
        if (NH > 1) { FOLD_RESIDENT(hoff); __syncthreads(); }
        FOLD_STORE(0);
        __syncthreads();
        if (half == 0) w1 = p.dbg ? wall_clock64() : 0;

        int cur = 0;
        for (int pr = pr_lo; pr <= pr_hi; ++pr) {
            const bool more = pr < pr_hi;
            if (more) FOLD_LOAD(pr + 1);
            const float* a_base = As + cur * FOLD2_M * S + wcol * 32 * S + frag;
            float4 af[KK];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) af[kk] = *reinterpret_cast<const float4*>(a_base + kk * 8);
            const int msb = 2 * pr - (oy0 + wrow) + p.pad + 1;      // merged slice of this wave's output row yy: msb - 4 yy
#pragma unroll
            for (int yy = 0; yy < RW; ++yy) {
                const int ms = msb - 4 * yy;
                if (ms >= 0 && ms <= p.KH) {               // wave-uniform
                    const float* b_base = Bs + ms * 32 * S + frag;
#pragma unroll
                    for (int kk = 0; kk < KK; ++kk) {
                        const float4 bf = *reinterpret_cast<const float4*>(b_base + kk * 8);
                        acc[yy] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].x, bf.x, acc[yy], 0, 0, 0);
                        acc[yy] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].y, bf.y, acc[yy], 0, 0, 0);
                        acc[yy] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].z, bf.z, acc[yy], 0, 0, 0);
                        acc[yy] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk].w, bf.w, acc[yy], 0, 0, 0);
                    }
                }
            }
            if (more) FOLD_STORE(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
        }

        const long long w2 = p.dbg ? wall_clock64() : 0;
        // ---- epilogue in four passes (pass hh: output rows oy0 + g + 4 hh of the four row groups): D tiles -> LDS [4][64][33],
        // then the diagonal sum over kx with the logical -> physical column map
        float* D = As;
        const size_t MO = (size_t)p.OH * p.OW;
        const int per_row = XO * p.COUT;
        // an output (row group g, channel c, column xo) of a pass is the same for all four passes: its index arithmetic (two divisions
        // by run-time values), bias and mean are formed once per tile instead of once per output
        constexpr int NE = 3;                      // 4 * per_row = 1440 outputs per pass on 512 threads (COUT = 3, XO = 120)
        int eg[NE], ec[NE], exo[NE]; float ebias[NE], emean[NE]; const float* ed[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            const int e = t + NT * k;
            const bool ok = e < 4 * per_row;
            const int g = ok ? e / per_row : 0, rem = ok ? e - g * per_row : 0;
            const int c = rem / XO, xo = rem - c * XO;
            eg[k] = ok && ox0 + xo < p.OW ? g : -1; ec[k] = c; exo[k] = xo;
            ebias[k] = p.bias[c]; emean[k] = c == 0 ? 103.939f : (c == 1 ? 116.779f : 123.68f);
            ed[k] = D + g * FOLD2_M * 33 + c * p.KW;
        }
#pragma unroll
        for (int hh = 0; hh < RW; ++hh) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int xr = wcol * 32 + (r & 3) + 8 * (r >> 2) + rbase;
                D[(wrow * FOLD2_M + xr) * 33 + col] = acc[hh][r];
            }
            __syncthreads();
            if (4 * per_row <= NE * NT) {
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    const int oy = oy0 + eg[k] + 4 * hh;
                    if (eg[k] < 0 || oy >= p.OH) continue;
                    float v = ebias[k];
                    for (int kx = 0; kx < p.KW; ++kx) v += ed[k][((exo[k] + kx) >> 1) * 33 + kx];
                    v = tanhf(v) * p.tanh_mul;                                          // models_video.lua:135-136
                    const size_t o = (size_t)oy * p.OW + ox0 + exo[k];
                    if (p.out_raw) p.out_raw[(size_t)ec[k] * MO + o] = v;
                    if (p.out_planar) p.out_planar[(size_t)(2 - ec[k]) * MO + o] = (v + emean[k]) / 255.f;      // preprocess.lua:66-71
                }
            } else {
            for (int e = t; e < 4 * per_row; e += NT) {
                const int g = e / per_row, rem = e - g * per_row;
                const int c = rem / XO, xo = rem - c * XO;
                const int oy = oy0 + g + 4 * hh, ox = ox0 + xo;
                if (oy >= p.OH || ox >= p.OW) continue;
                float v = p.bias[c];
                const float* d = D + g * FOLD2_M * 33 + c * p.KW;
                for (int kx = 0; kx < p.KW; ++kx) v += d[((xo + kx) >> 1) * 33 + kx];
                v = tanhf(v) * p.tanh_mul;                                              // models_video.lua:135-136
                const size_t o = (size_t)oy * p.OW + ox;
                if (p.out_raw) p.out_raw[(size_t)c * MO + o] = v;
                if (p.out_planar) {
                    const float mean = c == 0 ? 103.939f : (c == 1 ? 116.779f : 123.68f);
                    p.out_planar[(size_t)(2 - c) * MO + o] = (v + mean) / 255.f;          // preprocess.lua:66-71
                }
            }
            }
            __syncthreads();
        }
        if (p.dbg && t == 0) {
            long long* d = p.dbg + blockIdx.x * 8;
            d[0] += 1; d[1] += w1 - w0; d[2] += w2 - w1; d[3] += wall_clock64() - w2; d[4] += pr_hi - pr_lo + 1;
        }
    }
}

template <int CIN, int NH = 1>
int launch_fold_up2_t(FoldArgs a, int reserve_cus, hipStream_t st)
{
    const int S = CIN + 4;
    const size_t wbytes = (size_t)((a.KH + 1) * 32 * S + 4 * CIN) * sizeof(float);
    size_t stage = (size_t)(2 * FOLD2_M * S) * sizeof(float);
    const size_t epi = (size_t)4 * FOLD2_M * 33 * sizeof(float);
    if (epi > stage) stage = epi;
    const size_t lds = wbytes + stage;
    if (lds > 160 * 1024) { set_error("row-folded conv: %zu bytes of LDS needed", lds); return FAV_EUNSUPPORTED; }
    static PerDevice cache; int cus;
    FAV_HIP(launch_cus(cache, &cus, conv_rowfold_up2_kernel<CIN, NH>));
    const int XO = 2 * FOLD2_M - (a.KW - 1);
    a.tiles_x = (a.OW + XO - 1) / XO; a.tiles_y = (a.OH + FOLD_R - 1) / FOLD_R;
    const int tiles = a.tiles_x * a.tiles_y;
    const int nres = persistent_slots(cus, reserve_cus);
    static int dbg_n = diag_env("FAV_FOLD_DBG") ? atoi(diag_env("FAV_FOLD_DBG")) : 0;      // print the in-kernel timeline of the n-th launch
    const bool dbg = dbg_n > 0 && --dbg_n == 0;
    static long long* dbuf = nullptr;
    a.dbg = nullptr;
    if (dbg) { FAV_HIP(hipMalloc(reinterpret_cast<void**>(&dbuf), 512 * 8 * 8)); FAV_HIP(hipMemsetAsync(dbuf, 0, 512 * 8 * 8, st)); a.dbg = dbuf; }
    hipLaunchKernelGGL((conv_rowfold_up2_kernel<CIN, NH>), dim3(tiles < nres ? tiles : nres), dim3(512), lds, st, a);
    FAV_LAUNCH_CHECK("conv_rowfold_up2_kernel");
    if (dbg) {
        std::vector<long long> hb((size_t)512 * 8);
        FAV_HIP(hipStreamSynchronize(st)); FAV_HIP(hipMemcpy(hb.data(), dbuf, hb.size() * 8, hipMemcpyDeviceToHost));
        double n = 0, a0 = 0, a1 = 0, a2 = 0, rows = 0;
        for (int b = 0; b < 512; ++b) { n += hb[b * 8]; a0 += hb[b * 8 + 1]; a1 += hb[b * 8 + 2]; a2 += hb[b * 8 + 3]; rows += hb[b * 8 + 4]; }
        if (n > 0) fprintf(stderr, "FOLDDBG tiles=%.0f  per tile: first row %.2f  loop %.2f (%.1f staged rows)  epilogue %.2f us\n", n, a0 / n * 0.01, a1 / n * 0.01, rows / n, a2 / n * 0.01);
    }
    return FAV_OK;
}

template <int CIN>
int launch_fold_t(FoldArgs a, int reserve_cus, hipStream_t st)
{
    const int S = CIN + 4;
    const size_t wbytes = (size_t)(a.KH * 32 * S + 4 * CIN) * sizeof(float);      // resident: weights + transform table
    size_t stage = (size_t)(2 * FOLD_M * S) * sizeof(float);
    const size_t epi = (size_t)4 * FOLD_M * 33 * sizeof(float);                   // D tile of one epilogue pass
    if (epi > stage) stage = epi;
    const size_t lds = wbytes + stage;
    if (lds > 160 * 1024) { set_error("row-folded conv: %zu bytes of LDS needed", lds); return FAV_EUNSUPPORTED; }
    static PerDevice cache; int cus;
    FAV_HIP(launch_cus(cache, &cus, conv_rowfold_kernel<CIN>));
    const int XO = FOLD_M - (a.KW - 1);
    a.tiles_x = (a.OW + XO - 1) / XO; a.tiles_y = (a.OH + FOLD_R - 1) / FOLD_R;
    const int tiles = a.tiles_x * a.tiles_y;
    const int nres = persistent_slots(cus, reserve_cus);       // persistent blocks: leave the side queues their CUs
    hipLaunchKernelGGL((conv_rowfold_kernel<CIN>), dim3(tiles < nres ? tiles : nres), dim3(512), lds, st, a);
    FAV_LAUNCH_CHECK("conv_rowfold_kernel");
    return FAV_OK;
}

}  // namespace

bool conv_fold_eligible(const ConvShape& s)
{
    return !s.transposed && s.stride == 1 && s.cout * s.k <= 32 && s.k <= 9 &&
           (s.cin_pitch == 16 || s.cin_pitch == 32 || s.cin_pitch == 64 || s.cin_pitch == 128 || s.cin_pitch == 256);
}
// 128 / 256 input channels (checkpoints with more filters, README.md:141): only the form for a x2-upsampled input exists (U2 + c9s1-3,
// every architecture string of the reference ends that way); anything else with that many channels takes the generic kernel
bool conv_fold_launchable(int cin_pitch, int k, int pad, int ups, int IH, int IW)
{
    static const bool no_up2 = diag_env("FAV_NO_FOLD_UP2") != nullptr;
    if (cin_pitch <= 64) return true;
    return ups == 1 && !no_up2 && (pad & 1) == 0 && (k & 1) == 1 && (IH & 1) == 0 && (IW & 1) == 0 && k + 1 <= 10;
}

int launch_conv_fold(const ConvLaunch& c, hipStream_t st)
{
    FAV_REQUIRE(conv_fold_eligible(conv_shape(c)) && c.KH == c.KW && c.final_mode && c.wpk, "row-folded conv: not eligible");
    FoldArgs a;
    a.dbg = nullptr;
    a.in = c.in; a.wfold = c.wpk; a.bias = c.bias;
    a.scale1 = c.pre.scale1; a.shift1 = c.pre.shift1; a.scale2 = c.pre.scale2; a.shift2 = c.pre.shift2;
    a.stages = c.pre.stages; a.relu1 = c.pre.relu1; a.relu2 = c.pre.relu2;
    a.out_planar = c.out_planar; a.out_raw = c.out_raw_nchw;
    a.IH = c.IH; a.IW = c.IW; a.IWp = c.IWp; a.ups = c.ups; a.COUT = c.COUT; a.KH = c.KH; a.KW = c.KW; a.pad = c.pad;
    a.OH = c.OH; a.OW = c.OW; a.tanh_mul = c.tanh_mul;
    // x2 nearest-upsampled input: physical columns, merged ky slices (wfold carries them after the plain slices)
    static const bool no_up2 = diag_env("FAV_NO_FOLD_UP2") != nullptr;
    if (c.ups == 1 && !no_up2 && (c.pad & 1) == 0 && (c.KW & 1) == 1 && (c.IH & 1) == 0 && (c.IW & 1) == 0 && c.KH + 1 <= 10) {
        if (c.CIN == 256) return launch_fold_up2_t<64, 4>(a, c.reserve_cus, st);
        if (c.CIN == 128) return launch_fold_up2_t<64, 2>(a, c.reserve_cus, st);
        if (c.CIN == 64) return launch_fold_up2_t<64>(a, c.reserve_cus, st);
        if (c.CIN == 32) return launch_fold_up2_t<32>(a, c.reserve_cus, st);
    }
    FAV_REQUIRE(c.CIN <= 64, "row-folded conv: %d input channels are supported on a x2-upsampled input only", c.CIN);
    if (c.CIN == 64) return launch_fold_t<64>(a, c.reserve_cus, st);
    if (c.CIN == 32) return launch_fold_t<32>(a, c.reserve_cus, st);
    return launch_fold_t<16>(a, c.reserve_cus, st);
}

}  // namespace fav
