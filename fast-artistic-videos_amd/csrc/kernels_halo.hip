// kernels_halo.hip -- the halo-resident 3x3 stride-1 kernels, fp32 and bf16 operands (conv3_halo_kernel, conv3_halo_bf16_kernel).
// The stride-2 member of the family is in kernels_halo_s2.hip.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "fav_internal.h"
#include "conv_device.h"
#include "launch_common.h"

namespace fav {

// ------------------------------------------------------------------------------------------------
// 3x3 stride-1 layers (the ten 128->128 residual convolutions and c3s1-64: 71 % of the network's FLOPs):
// halo-resident implicit GEMM.  The generic kernel re-gathers (and re-transforms) its activation operand
// for every tap; measured, that global gather costs ~20 % of the kernel.  Here a block (8 waves, one per
// CU, stream-K over all (tile, K-step) units) owns an 8 x 32 pixel output tile; for each 32-channel slice
// the (8+2) x (32+2) pixel halo is gathered ONCE, transformed (producer's IN/ReLU stages, x2 nearest
// upsample, zero padding) and kept in LDS, and the 9 taps read their A fragments straight from it with
// conflict-free ds_read_b128 (a wave = one output row of 32 pixels, so the fragment rows are 32 consecutive
// halo pixels).  Only the weight slice (BN x 32 per step) streams through LDS.  Global->LDS traffic per
// MFMA drops 3x.  K order = (channel slice, tap, 32 channels): the same repacked weights as the generic
// kernel.  Epilogue as the generic kernel (bias, NHWC store, per-tile IN partials with explicit counts).
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int H3_TH = 8, H3_TW = 32;   // output tile: 8 rows (one per wave) x 32 pixels

struct H3Args {
    const float* in; const float* wgt; const float* bias;
    const float* scale1; const float* shift1; const float* scale2; const float* shift2;
    float* out; float2* partials; int* counts;
    float* sk_ws; unsigned* sk_flags; unsigned sk_epoch; unsigned* sk_err;
    int IH, IW, IWp, ups, CIN, COUT, COUTp, pad, OH, OW, Kpad, tiles_x, tiles_y;
    int nb;                  // number of 16 x 16 edge tiles (fp32 kernel; see conv3_halo_tiles)
    int stages, relu1, relu2;
    const unsigned short* wgt16;   // bf16 copy of the weights (fast mode) or null
    long long* dbg;          // optional in-kernel timeline (FAV_H3_DBG), 24 slots per block
};

// fp32 MFMA and the vector ALU do not overlap on a SIMD (measured: scripts/mfma_mix.hip -- every VALU instruction in the
// loop costs its issue cycles in matrix throughput), so the K loop is built to need almost none:
//   * the nine taps of a channel slice are unrolled: tap offsets, the weight ring slot (tap % 3) and the halo piece index
//     are compile-time constants, i.e. immediate offsets on per-thread base registers that are set once per tile/slice
//   * global addresses are scalar base (advanced by the scalar ALU) + a per-thread 32-bit offset fixed for the tile
//   * what is left per step: the IN/ReLU transform of one 16-byte halo piece (6 of 9 steps)
// Software pipeline of one K step (32 channels of one tap; 4 fragment groups of 8 channels):
//   start  : weights of step s+1 (in registers since step s-1) -> LDS ring slot (s+1)%3; issue the global load of step
//            s+2's weights and of one sixth of the NEXT channel slice's halo
//   groups : the A/B fragments of group g+1 are read from LDS into the other register set while group g's 16 MFMAs issue;
//            the last group prefetches group 0 of step s+1, so no LDS latency is exposed in the steady state
//   barrier: one per step, between groups 1 and 2 -- it publishes ring slot (s+1)%3 half a step before its first read
//            and is never followed by a dependent LDS read (three slots make the write-after-read side safe)
//   end    : the halo piece, transformed, -> the other halo buffer
template <int BN, bool S2>
__global__ __launch_bounds__(512, 2) void conv3_halo_kernel(const H3Args p)
{
    constexpr int NT = 512;
    constexpr int HWD = H3_TW + 2, HP = (H3_TH + 2) * HWD;        // 34, 340 halo pixels
    constexpr int TN = BN / 32;
    constexpr int NHV = (HP * 8 + NT - 1) / NT;                   // 16-byte halo pieces per thread per slice (6)
    constexpr int ALIAS = NT * NHV - HP * 8;                       // units past the end alias earlier ones (same data, same slot)
    constexpr int BROWS = BN / 64;                                 // weight rows per thread per step
    static_assert(NHV == 6, "two halo pieces per tap row");
    static_assert(ALIAS % 8 == 0 && ALIAS <= NT, "halo aliasing");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Hs = smem;                           // [2][HP][LDSS]
    float* Bs = Hs + 2 * HP * LDSS;             // [3][BN][LDSS]
    float* aff = Bs + 3 * BN * LDSS;            // [4][CIN]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int CIN = p.CIN;
    const int nchunks = CIN >> 5, nsteps = nchunks * 9;
    // Tiles.  A: 8 rows x 32 columns, wave = one row (tiles_x columns of them, tiles_y rows).  B (p.nb > 0): the ragged right
    // edge -- fewer than 17 columns wide -- is cut into 16 x 16 tiles instead, wave = TWO rows of 16 pixels: half as many edge
    // tiles, each fully used in x.  The 18 x 18 halo of a B tile (324 pixels, pitch 18) fits the same buffers.
    const int na = p.tiles_x * p.tiles_y, ntiles = na + p.nb;

    int dbi = 0;
#define DBG_T() { if (p.dbg && t == 0 && dbi < 22) p.dbg[blockIdx.x * 24 + dbi++] = wall_clock64(); }
    DBG_T();
    const int lb = xcd_linear_block();
    for (int i = t; i < CIN; i += NT) {
        aff[i] = p.stages >= 1 ? p.scale1[i] : 1.f; aff[CIN + i] = p.stages >= 1 ? p.shift1[i] : 0.f;
        aff[2 * CIN + i] = p.stages >= 2 ? p.scale2[i] : 1.f; aff[3 * CIN + i] = p.stages >= 2 ? p.shift2[i] : 0.f;
    }
    const float lo1 = (p.stages >= 1 && p.relu1) ? 0.f : -INFINITY;
    const float lo2 = (p.stages >= 2 && p.relu2) ? 0.f : -INFINITY;
    __syncthreads();

    const int c4 = t & 7, r0 = t >> 3;                      // staging: weight row r0 (+64) / halo pixel r0 (+64 i), 16-byte chunk c4
    const int frag_k = (lane >> 5) * 4;                     // k pair {r, 4+r} by half-wave
    const int m = lane & 31;
    const int col = lane & 31, rbase = 4 * (lane >> 5);
    // per-thread bases; everything else in the K loop is an immediate or a scalar
    const unsigned wofs = (unsigned)(r0 * p.Kpad + c4 * 4) * 4u;            // byte offset of this thread's weight chunk in a step
    const unsigned wrow64 = (unsigned)(64 * p.Kpad) * 4u;
    float* const bst = Bs + r0 * LDSS + c4 * 4;                             // weight staging slot
    float* const hst = Hs + r0 * LDSS + c4 * 4;                             // halo staging slot of piece 0, buffer 0
    constexpr int HWB = 18, HPB = HWB * HWB, ALIASB = NT * NHV - HPB * 8;    // B tiles: 18 x 18 halo
    static_assert(ALIASB % 8 == 0 && ALIASB <= NT, "halo aliasing (B tiles)");
    const int hst_lastA = (t + NT * (NHV - 1) >= HP * 8) ? (NT * (NHV - 1) - ALIAS) / 8 * LDSS : 64 * (NHV - 1) * LDSS;
    const int hst_lastB = (t + NT * (NHV - 1) >= HPB * 8) ? (NT * (NHV - 1) - ALIASB) / 8 * LDSS : 64 * (NHV - 1) * LDSS;
    const float* const afrA = Hs + (wave * HWD + m) * LDSS + frag_k;        // A fragments: tap (0,0), buffer 0
    // B tiles: lanes 0-15 = row 2w, lanes 16-31 = row 2w+1 with the columns rotated by 14 -- the 16 pixels a ds_read_b128 lane
    // group touches must differ mod 16 (row stride 36 floats), and the second row starts 18 pixels after the first
    const int colB = m < 16 ? m : ((m + 14) & 15);
    const float* const afrB = Hs + ((2 * wave + (m >> 4)) * HWB + colB) * LDSS + frag_k;
    const float* const bfr = Bs + m * LDSS + frag_k;                        // B fragments: ring slot 0
    const float* const affr = aff + c4 * 4;

    // stream-K work unit: one tap row (3 K steps) of one channel slice of one tile.  Inside a unit kx, the weight ring
    // slot (= kx) and the position of the halo pieces are compile-time constants; ky and the slice are scalars.
    const int nunits = nchunks * 3;
    const int U = ntiles * nunits;
    int u = (int)((long long)U * lb / gridDim.x);
    const int u_end = (int)((long long)U * (lb + 1) / gridDim.x);

    while (u < u_end) {
        const int tile = u / nunits;
        const int k0 = u - tile * nunits;
        const int k1 = (u_end - u) < nunits - k0 ? k0 + (u_end - u) : nunits;
        u += k1 - k0;
        const bool tb = tile >= na;                                   // B tile (uniform)
        const int ty = tb ? tile - na : tile / p.tiles_x, tx = tb ? p.tiles_x : tile - ty * p.tiles_x;
        const int oy0 = ty * (tb ? 16 : H3_TH), ox0 = tx * H3_TW;
        const int hwd = tb ? HWB : HWD;
        const int hst_last = tb ? hst_lastB : hst_lastA;
        const float* const afr = tb ? afrB : afrA;
        DBG_T();   /* work item start */

        // halo piece i: unit e = t + 512*i -> halo pixel e>>3, channel chunk e&7; per tile: byte offset (chunk 0 if outside) and mask
        int hoff[NHV]; float hmask[NHV];
#pragma unroll
        for (int i = 0; i < NHV; ++i) {
            int e = t + NT * i; e -= e >= (tb ? HPB : HP) * 8 ? (tb ? ALIASB : ALIAS) : 0;
            const int pix = e >> 3, hy = tb ? (pix * 3641) >> 16 : (pix * 1928) >> 16, hx = pix - hy * hwd;      // pix / 18, pix / 34
            const int iy = oy0 - p.pad + hy, ix = ox0 - p.pad + hx;
            const bool v = ((unsigned)iy < (unsigned)p.IH) & ((unsigned)ix < (unsigned)p.IW);
            hoff[i] = ((v ? ((iy >> p.ups) * p.IWp + (ix >> p.ups)) * CIN : 0) + c4 * 4) * 4;
            hmask[i] = v ? 1.f : 0.f;
        }
        const int c_first = (k0 * 21846) >> 16, ky0 = k0 - c_first * 3;      // k / 3
        const int c_last = ((k1 - 1) * 21846) >> 16;

        float4 hr; float hm; v4f rb[BROWS];
        v4f sc1, sh1, sc2, sh2;             // IN/ReLU stages of the slice being staged, this thread's 4 channels
#define H3_AFF(chunk_)                                                                              \
        { sc1 = *reinterpret_cast<const v4f*>(affr + (chunk_) * 32); sh1 = *reinterpret_cast<const v4f*>(affr + CIN + (chunk_) * 32); \
          if (S2) { sc2 = *reinterpret_cast<const v4f*>(affr + 2 * CIN + (chunk_) * 32); sh2 = *reinterpret_cast<const v4f*>(affr + 3 * CIN + (chunk_) * 32); } }
#define H3_XFORM(v_, m_)                                                                            \
        { v_.x = fmaxf(fmaf(v_.x, sc1.x, sh1.x), lo1); v_.y = fmaxf(fmaf(v_.y, sc1.y, sh1.y), lo1);  \
          v_.z = fmaxf(fmaf(v_.z, sc1.z, sh1.z), lo1); v_.w = fmaxf(fmaf(v_.w, sc1.w, sh1.w), lo1);  \
          if (S2) { v_.x = fmaxf(fmaf(v_.x, sc2.x, sh2.x), lo2); v_.y = fmaxf(fmaf(v_.y, sc2.y, sh2.y), lo2); \
                    v_.z = fmaxf(fmaf(v_.z, sc2.z, sh2.z), lo2); v_.w = fmaxf(fmaf(v_.w, sc2.w, sh2.w), lo2); } \
          v_.x *= m_; v_.y *= m_; v_.z *= m_; v_.w *= m_; }
#define H3_HLDS(i_) ((i_) == NHV - 1 ? hst_last : 64 * (i_) * LDSS)
#define H3_LOAD_B(src_)                                                                             \
        { _Pragma("unroll") for (int j = 0; j < BROWS; ++j) rb[j] = *reinterpret_cast<const v4f*>(reinterpret_cast<const char*>(src_) + (wofs + j * wrow64)); }
#define H3_STORE_B(slot_)                                                                           \
        { _Pragma("unroll") for (int j = 0; j < BROWS; ++j) *reinterpret_cast<v4f*>(bst + ((slot_) * BN + 64 * j) * LDSS) = rb[j]; }

        {
            // prologue: this slice's whole halo -> buffer 0; the pieces of the next slice that the skipped tap rows would
            // have staged -> buffer 1; all loads in flight before the first store
            const char* in0 = reinterpret_cast<const char*>(p.in + c_first * 32);
            const char* in1 = reinterpret_cast<const char*>(p.in + min(c_first + 1, c_last) * 32);
            float4 q0[NHV], q1[NHV];
#pragma unroll
            for (int i = 0; i < NHV; ++i) q0[i] = *reinterpret_cast<const float4*>(in0 + hoff[i]);
            H3_LOAD_B(p.wgt + k0 * 3 * BK);
#pragma unroll
            for (int i = 0; i < NHV; ++i) if (i < 2 * ky0) q1[i] = *reinterpret_cast<const float4*>(in1 + hoff[i]);
            H3_AFF(c_first);
#pragma unroll
            for (int i = 0; i < NHV; ++i) { H3_XFORM(q0[i], hmask[i]); *reinterpret_cast<float4*>(hst + H3_HLDS(i)) = q0[i]; }
            H3_STORE_B(0);
            H3_LOAD_B(p.wgt + min(k0 * 3 + 1, nsteps - 1) * BK);
            H3_AFF(min(c_first + 1, c_last));
#pragma unroll
            for (int i = 0; i < NHV; ++i) if (i < 2 * ky0) { H3_XFORM(q1[i], hmask[i]); *reinterpret_cast<float4*>(hst + HP * LDSS + H3_HLDS(i)) = q1[i]; }
        }
        f32x16 acc[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        __syncthreads();

        v4f fa[2], fb[2][TN];
#define H3_FRAG(set_, ap_, bp_)                                                                     \
        { fa[set_] = *reinterpret_cast<const v4f*>(ap_);                                            \
          _Pragma("unroll") for (int j = 0; j < TN; ++j) fb[set_][j] = *reinterpret_cast<const v4f*>((bp_) + j * 32 * LDSS); }
#define H3_MFMA(set_)                                                                               \
        { _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                          \
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_].x, fb[set_][j].x, acc[j], 0, 0, 0); \
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_].y, fb[set_][j].y, acc[j], 0, 0, 0); \
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_].z, fb[set_][j].z, acc[j], 0, 0, 0); \
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_].w, fb[set_][j].w, acc[j], 0, 0, 0); } }
#define H3_GROUP(nds_)                                                                              \
        { __builtin_amdgcn_sched_group_barrier(0x100, nds_, 0); __builtin_amdgcn_sched_group_barrier(0x008, 4 * TN, 0); }
        // one K step, kx = KX (compile time).  a_cu = A fragments of this tap row, a_nu = of the next unit's; the halo
        // piece staged in this step (KX < 2) is piece 2*ky + KX of the next slice
#define H3_STEP(KX)                                                                                 \
        {   constexpr int NB = ((KX) + 1) % 3;                                                      \
            const float* an_ = (KX) == 2 ? a_nu : a_cu + ((KX) + 1) * LDSS;                         \
            H3_FRAG(1, a_cu + (KX) * LDSS + 8, bfr + (KX) * BN * LDSS + 8);                         \
            H3_STORE_B(NB);                                                                         \
            H3_LOAD_B(p.wgt + min(sg + (KX) + 2, nsteps - 1) * BK);                                 \
            if ((KX) < 2) { hr = *reinterpret_cast<const float4*>(in_n + ((KX) == 0 ? ho0 : ho1)); hm = (KX) == 0 ? hm0 : hm1; } \
            H3_MFMA(0); H3_GROUP(1 + TN);                                                           \
            H3_FRAG(0, a_cu + (KX) * LDSS + 16, bfr + (KX) * BN * LDSS + 16); H3_MFMA(1); H3_GROUP(1 + TN); \
            __syncthreads();                                                                        \
            H3_FRAG(1, a_cu + (KX) * LDSS + 24, bfr + (KX) * BN * LDSS + 24); H3_MFMA(0); H3_GROUP(1 + TN); \
            H3_FRAG(0, an_, bfr + NB * BN * LDSS);                                                  \
            if ((KX) < 2) { H3_XFORM(hr, hm); *reinterpret_cast<float4*>(h_nx + ((KX) == 0 ? hl0 : hl1)) = hr; } \
            H3_MFMA(1); H3_GROUP(1 + TN);                                                           \
        }

        H3_FRAG(0, afr + ky0 * hwd * LDSS, bfr);           // fragments of the first step's group 0
        DBG_T();   /* loop start */
        const long long ck0 = p.dbg ? clock64() : 0, wk0 = p.dbg ? wall_clock64() : 0;
        int c = c_first, ky = ky0, par = 0;
        for (int uu = k0; uu < k1; ++uu) {
            const float* a_cu = afr + (par * HP + ky * hwd) * LDSS;
            const float* a_nu = ky == 2 ? afr + (par ^ 1) * (HP * LDSS) : a_cu + hwd * LDSS;
            float* h_nx = hst + (par ^ 1) * (HP * LDSS);
            const int cn = min(c + 1, c_last);                              // no next slice: the pieces land in the unused buffer
            const char* in_n = reinterpret_cast<const char*>(p.in + cn * 32);
            const int sg = uu * 3;
            // the two halo pieces of this unit: 2*ky and 2*ky + 1 (uniform selects)
            const int ho0 = ky == 0 ? hoff[0] : (ky == 1 ? hoff[2] : hoff[4]), ho1 = ky == 0 ? hoff[1] : (ky == 1 ? hoff[3] : hoff[5]);
            const float hm0 = ky == 0 ? hmask[0] : (ky == 1 ? hmask[2] : hmask[4]), hm1 = ky == 0 ? hmask[1] : (ky == 1 ? hmask[3] : hmask[5]);
            const int hl0 = 128 * ky * LDSS, hl1 = ky == 2 ? hst_last : (128 * ky + 64) * LDSS;
            H3_AFF(cn);
            H3_STEP(0) H3_STEP(1) H3_STEP(2)
            if (++ky == 3) { ky = 0; ++c; par ^= 1; }
        }
        __syncthreads();                    // the epilogue reuses the staging memory
        DBG_T();   /* loop end */
        if (p.dbg && t == 0 && k1 - k0 > 6) { p.dbg[blockIdx.x * 24 + 21] = clock64() - ck0; p.dbg[blockIdx.x * 24 + 22] = wall_clock64() - wk0; p.dbg[blockIdx.x * 24 + 20] = (k1 - k0) * 3; }
#undef H3_AFF
#undef H3_XFORM
#undef H3_HLDS
#undef H3_LOAD_B
#undef H3_STORE_B
#undef H3_FRAG
#undef H3_MFMA
#undef H3_GROUP
#undef H3_STEP

        // ------------------------------------------------------------ stream-K hand-off (see conv_mfma_kernel)
        constexpr int NV4 = TN * 4;
        if (k0 > 0) {
            float4* slot = reinterpret_cast<float4*>(p.sk_ws) + (size_t)lb * NV4 * NT + t;
            // write-through payload -> drained -> sc1 flag (no L2 write-back fence)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    store16_wt(slot + (size_t)(j * 4 + q) * NT, v4f{acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]});
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (t == 0) __hip_atomic_store(p.sk_flags + lb, p.sk_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            DBG_T(); DBG_T();
            continue;
        }
        if (k1 < nunits) {
            int covered = k1;
            for (int nb = lb + 1; covered < nunits && nb < (int)gridDim.x; ++nb) {
                const int nu0 = (int)((long long)U * nb / gridDim.x), nu1 = (int)((long long)U * (nb + 1) / gridDim.x);
                const int span = (nu1 - nu0) < (nunits - covered) ? (nu1 - nu0) : (nunits - covered);
                if (t == 0) {
                    unsigned spins = 0;
                    while (__hip_atomic_load(p.sk_flags + nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != p.sk_epoch) {
                        __builtin_amdgcn_s_sleep(4);
                        if (++spins > (1u << 22)) { if (p.sk_err) __hip_atomic_store(p.sk_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                }
                __syncthreads();
                const float4* slot = reinterpret_cast<const float4*>(p.sk_ws) + (size_t)nb * NV4 * NT + t;
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 v = slot[(size_t)(j * 4 + q) * NT];
                        acc[j][4 * q] += v.x; acc[j][4 * q + 1] += v.y; acc[j][4 * q + 2] += v.z; acc[j][4 * q + 3] += v.w;
                    }
                covered += span;
            }
        }

        DBG_T();   /* fixup end */
        // ------------------------------------------------------------ epilogue: wave = output row, MFMA rows = columns
        float* red = smem;                 // [8][BN] float2 + [8] int
        // output pixel of MFMA row mi: A tiles (oy0 + wave, ox0 + mi); B tiles (oy0 + 2 wave + mi / 16, ox0 + un-rotated column)
#define H3_OPIX(r_)                                                                                 \
        const int mi_ = ((r_) & 3) + 8 * ((r_) >> 2) + rbase;                                       \
        const int oy = tb ? oy0 + 2 * wave + (mi_ >> 4) : oy0 + wave;                               \
        const int ox = tb ? ox0 + (mi_ < 16 ? mi_ : ((mi_ + 14) & 15)) : ox0 + mi_;                 \
        const bool ok_ = tb ? (oy < p.OH) & (ox < p.OW) & ((mi_ < 16 ? mi_ : ((mi_ + 14) & 15)) < 16) : (oy < p.OH) & (ox < p.OW);
        float lsum[TN]; int lcnt = 0;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = j * 32 + col;
            const float bv = p.bias[n];
            float sm = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                H3_OPIX(r);
                const float v = acc[j][r] + bv;
                acc[j][r] = v;
                if (ok_) {
                    if (n < p.COUT) p.out[((size_t)oy * p.OW + ox) * p.COUT + n] = v;
                    sm += v;
                    if (j == 0) ++lcnt;
                }
            }
            lsum[j] = sm;
        }
        if (p.partials != nullptr) {
            float2* st = reinterpret_cast<float2*>(red);          // [8 waves][BN]
            int* wn = reinterpret_cast<int*>(red + 16 * BN);        // [8]
            const int nw = lcnt + __shfl_xor(lcnt, 32);             // valid pixels of this wave's 32
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float sm = lsum[j] + __shfl_xor(lsum[j], 32);
                const float mu = nw ? sm / (float)nw : 0.f;
                float q = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    H3_OPIX(r);
                    const float d = acc[j][r] - mu;
                    if (ok_) q = fmaf(d, d, q);
                }
                q += __shfl_xor(q, 32);
                if (lane < 32) st[wave * BN + j * 32 + lane] = make_float2(mu, q);
            }
            if (lane == 0) wn[wave] = nw;
            __syncthreads();
            if (t < BN) {
                int n;
                p.partials[(size_t)tile * p.COUTp + t] = merge_wave_stats(st, wn, 8, BN, t, &n);
                if (t == 0) p.counts[tile] = n;
            }
        }
#undef H3_OPIX
        __syncthreads();
        DBG_T();   /* epilogue end */
    }
    if (p.dbg && t == 0) p.dbg[blockIdx.x * 24 + 23] = dbi;
#undef DBG_T
}

// ------------------------------------------------------------------------------------------------
// Optional fast mode (NOT the parity mode): the same halo-resident kernel with the two operands rounded to
// bf16 on their way into LDS (activations after the pending IN/ReLU transform, weights pre-rounded on the host) and
// v_mfma_f32_32x32x16_bf16 (fp32 accumulation, fp32 activations in HBM).  One K step = 2 matrix instructions per 32x32 tile
// instead of 16, so the kernel turns from MFMA-bound into staging-bound.  Selected per network with fav_net_set_precision.
// ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int BN, bool S2>
__global__ __launch_bounds__(512, 2) void conv3_halo_bf16_kernel(const H3Args p)
{
    constexpr int NT = 512;
    constexpr int HWD = H3_TW + 2, HP = (H3_TH + 2) * HWD;        // 34, 340 halo pixels
    constexpr int TN = BN / 32;
    constexpr int NHV = (HP * 8 + NT - 1) / NT;                   // 16-byte halo pieces per thread per slice (6)
    constexpr int ALIAS = NT * NHV - HP * 8;                       // units past the end alias earlier ones (same data, same slot)
    static_assert(NHV == 6, "two halo pieces per tap row");
    static_assert(ALIAS % 8 == 0 && ALIAS <= NT, "halo aliasing");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LB = 40;                      // LDS row stride in bf16 units: 32 channels + 8 pad = 80 bytes (conflict-free ds_read_b128)
    unsigned short* Hs = reinterpret_cast<unsigned short*>(smem);    // [2][HP][LB]   bf16
    unsigned short* Bs = Hs + 2 * HP * LB;                           // [3][BN][LB]   bf16
    float* aff = reinterpret_cast<float*>(Bs + 3 * BN * LB);         // [4][CIN]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int CIN = p.CIN;
    const int nchunks = CIN >> 5, nsteps = nchunks * 9;
    const int ntiles = p.tiles_x * p.tiles_y;

    int dbi = 0;
#define DBG_T() { if (p.dbg && t == 0 && dbi < 22) p.dbg[blockIdx.x * 24 + dbi++] = wall_clock64(); }
    DBG_T();
    const int lb = xcd_linear_block();
    for (int i = t; i < CIN; i += NT) {
        aff[i] = p.stages >= 1 ? p.scale1[i] : 1.f; aff[CIN + i] = p.stages >= 1 ? p.shift1[i] : 0.f;
        aff[2 * CIN + i] = p.stages >= 2 ? p.scale2[i] : 1.f; aff[3 * CIN + i] = p.stages >= 2 ? p.shift2[i] : 0.f;
    }
    const float lo1 = (p.stages >= 1 && p.relu1) ? 0.f : -INFINITY;
    const float lo2 = (p.stages >= 2 && p.relu2) ? 0.f : -INFINITY;
    __syncthreads();

    const int c4 = t & 7, r0 = t >> 3;                      // staging: weight row r0 (+64) / halo pixel r0 (+64 i), 16-byte chunk c4
    const int frag_k = (lane >> 5) * 8;                     // 8 consecutive channels per half-wave (one 32x32x16 operand)
    const int m = lane & 31;
    const int col = lane & 31, rbase = 4 * (lane >> 5);
    // per-thread bases; everything else in the K loop is an immediate or a scalar
    const int wr = t >> 2, wc = t & 3;                                      // weight staging: row wr, 16-byte chunk wc (8 bf16)
    const bool wact = wr < BN;
    const unsigned wofs = (unsigned)(wr * p.Kpad + wc * 8) * 2u;            // byte offset of this thread's weight chunk in a step
    unsigned short* const bst = Bs + wr * LB + wc * 8;                      // weight staging slot
    unsigned short* const hst = Hs + r0 * LB + c4 * 4;                      // halo staging slot of piece 0, buffer 0 (4 bf16 = 8 bytes)
    const int hst_last = (t + NT * (NHV - 1) >= HP * 8) ? (NT * (NHV - 1) - ALIAS) / 8 * LB : 64 * (NHV - 1) * LB;
    const unsigned short* const afr = Hs + (wave * HWD + m) * LB + frag_k;  // A fragments: tap (0,0), buffer 0
    const unsigned short* const bfr = Bs + m * LB + frag_k;                 // B fragments: ring slot 0
    const float* const affr = aff + c4 * 4;

    // stream-K work unit: one tap row (3 K steps) of one channel slice of one tile.  Inside a unit kx, the weight ring
    // slot (= kx) and the position of the halo pieces are compile-time constants; ky and the slice are scalars.
    const int nunits = nchunks * 3;
    const int U = ntiles * nunits;
    int u = (int)((long long)U * lb / gridDim.x);
    const int u_end = (int)((long long)U * (lb + 1) / gridDim.x);

    while (u < u_end) {
        const int tile = u / nunits;
        const int k0 = u - tile * nunits;
        const int k1 = (u_end - u) < nunits - k0 ? k0 + (u_end - u) : nunits;
        u += k1 - k0;
        const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        const int oy0 = ty * H3_TH, ox0 = tx * H3_TW;
        DBG_T();   /* work item start */

        // halo piece i: unit e = t + 512*i -> halo pixel e>>3, channel chunk e&7; per tile: byte offset (chunk 0 if outside) and mask
        int hoff[NHV]; float hmask[NHV];
#pragma unroll
        for (int i = 0; i < NHV; ++i) {
            int e = t + NT * i; e -= e >= HP * 8 ? ALIAS : 0;
            const int pix = e >> 3, hy = (pix * 1928) >> 16, hx = pix - hy * HWD;
            const int iy = oy0 - p.pad + hy, ix = ox0 - p.pad + hx;
            const bool v = ((unsigned)iy < (unsigned)p.IH) & ((unsigned)ix < (unsigned)p.IW);
            hoff[i] = ((v ? ((iy >> p.ups) * p.IWp + (ix >> p.ups)) * CIN : 0) + c4 * 4) * 4;
            hmask[i] = v ? 1.f : 0.f;
        }
        const int c_first = (k0 * 21846) >> 16, ky0 = k0 - c_first * 3;      // k / 3
        const int c_last = ((k1 - 1) * 21846) >> 16;

        float4 hr; float hm; v4f rb;
        v4f sc1, sh1, sc2, sh2;             // IN/ReLU stages of the slice being staged, this thread's 4 channels
#define H3_AFF(chunk_)                                                                              \
        { sc1 = *reinterpret_cast<const v4f*>(affr + (chunk_) * 32); sh1 = *reinterpret_cast<const v4f*>(affr + CIN + (chunk_) * 32); \
          if (S2) { sc2 = *reinterpret_cast<const v4f*>(affr + 2 * CIN + (chunk_) * 32); sh2 = *reinterpret_cast<const v4f*>(affr + 3 * CIN + (chunk_) * 32); } }
#define H3_XFORM(v_, m_)                                                                            \
        { v_.x = fmaxf(fmaf(v_.x, sc1.x, sh1.x), lo1); v_.y = fmaxf(fmaf(v_.y, sc1.y, sh1.y), lo1);  \
          v_.z = fmaxf(fmaf(v_.z, sc1.z, sh1.z), lo1); v_.w = fmaxf(fmaf(v_.w, sc1.w, sh1.w), lo1);  \
          if (S2) { v_.x = fmaxf(fmaf(v_.x, sc2.x, sh2.x), lo2); v_.y = fmaxf(fmaf(v_.y, sc2.y, sh2.y), lo2); \
                    v_.z = fmaxf(fmaf(v_.z, sc2.z, sh2.z), lo2); v_.w = fmaxf(fmaf(v_.w, sc2.w, sh2.w), lo2); } \
          v_.x *= m_; v_.y *= m_; v_.z *= m_; v_.w *= m_; }
#define H3_HLDS(i_) ((i_) == NHV - 1 ? hst_last : 64 * (i_) * LB)
#define H3_PUT(dst_, v_) { const bf16x2 lo_ = __builtin_convertvector(f32x2{v_.x, v_.y}, bf16x2), hi_ = __builtin_convertvector(f32x2{v_.z, v_.w}, bf16x2); \
                         uint2 w_; w_.x = __builtin_bit_cast(unsigned, lo_); w_.y = __builtin_bit_cast(unsigned, hi_); *reinterpret_cast<uint2*>(dst_) = w_; }
#define H3_LOAD_B(src_)  { if (wact) rb = *reinterpret_cast<const v4f*>(reinterpret_cast<const char*>(src_) + wofs); }
#define H3_STORE_B(slot_) { if (wact) *reinterpret_cast<v4f*>(bst + (slot_) * BN * LB) = rb; }

        {
            // prologue: this slice's whole halo -> buffer 0; the pieces of the next slice that the skipped tap rows would
            // have staged -> buffer 1; all loads in flight before the first store
            const char* in0 = reinterpret_cast<const char*>(p.in + c_first * 32);
            const char* in1 = reinterpret_cast<const char*>(p.in + min(c_first + 1, c_last) * 32);
            float4 q0[NHV], q1[NHV];
#pragma unroll
            for (int i = 0; i < NHV; ++i) q0[i] = *reinterpret_cast<const float4*>(in0 + hoff[i]);
            H3_LOAD_B(p.wgt16 + k0 * 3 * BK);
#pragma unroll
            for (int i = 0; i < NHV; ++i) if (i < 2 * ky0) q1[i] = *reinterpret_cast<const float4*>(in1 + hoff[i]);
            H3_AFF(c_first);
#pragma unroll
            for (int i = 0; i < NHV; ++i) { H3_XFORM(q0[i], hmask[i]); H3_PUT(hst + H3_HLDS(i), q0[i]); }
            H3_STORE_B(0);
            H3_LOAD_B(p.wgt16 + min(k0 * 3 + 1, nsteps - 1) * BK);
            H3_AFF(min(c_first + 1, c_last));
#pragma unroll
            for (int i = 0; i < NHV; ++i) if (i < 2 * ky0) { H3_XFORM(q1[i], hmask[i]); H3_PUT(hst + HP * LB + H3_HLDS(i), q1[i]); }
        }
        f32x16 acc[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        __syncthreads();

        bf16x8 fa[2], fb[2][TN];
#define H3_FRAG(set_, ap_, bp_)                                                                     \
        { fa[set_] = *reinterpret_cast<const bf16x8*>(ap_);                                         \
          _Pragma("unroll") for (int j = 0; j < TN; ++j) fb[set_][j] = *reinterpret_cast<const bf16x8*>((bp_) + j * 32 * LB); }
#define H3_MFMA(set_)                                                                               \
        { _Pragma("unroll") for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set_], fb[set_][j], acc[j], 0, 0, 0); }
#define H3_GROUP(nds_)                                                                              \
        { __builtin_amdgcn_sched_group_barrier(0x100, nds_, 0); __builtin_amdgcn_sched_group_barrier(0x008, TN, 0); }
        // one K step (32 channels of one tap = two 16-channel MFMA groups), kx = KX (compile time)
#define H3_STEP(KX)                                                                                 \
        {   constexpr int NB = ((KX) + 1) % 3;                                                      \
            const unsigned short* an_ = (KX) == 2 ? a_nu : a_cu + ((KX) + 1) * LB;                  \
            H3_FRAG(1, a_cu + (KX) * LB + 16, bfr + (KX) * BN * LB + 16);                           \
            H3_STORE_B(NB);                                                                         \
            H3_LOAD_B(p.wgt16 + min(sg + (KX) + 2, nsteps - 1) * BK);                               \
            if ((KX) < 2) { hr = *reinterpret_cast<const float4*>(in_n + ((KX) == 0 ? ho0 : ho1)); hm = (KX) == 0 ? hm0 : hm1; } \
            H3_MFMA(0); H3_GROUP(1 + TN);                                                           \
            __syncthreads();                                                                        \
            H3_FRAG(0, an_, bfr + NB * BN * LB);                                                    \
            if ((KX) < 2) { H3_XFORM(hr, hm); H3_PUT(h_nx + ((KX) == 0 ? hl0 : hl1), hr); }         \
            H3_MFMA(1); H3_GROUP(1 + TN);                                                           \
        }

        H3_FRAG(0, afr + ky0 * HWD * LB, bfr);             // fragments of the first step's first group
        DBG_T();   /* loop start */
        const long long ck0 = p.dbg ? clock64() : 0, wk0 = p.dbg ? wall_clock64() : 0;
        int c = c_first, ky = ky0, par = 0;
        for (int uu = k0; uu < k1; ++uu) {
            const unsigned short* a_cu = afr + (par * HP + ky * HWD) * LB;
            const unsigned short* a_nu = ky == 2 ? afr + (par ^ 1) * (HP * LB) : a_cu + HWD * LB;
            unsigned short* h_nx = hst + (par ^ 1) * (HP * LB);
            const int cn = min(c + 1, c_last);                              // no next slice: the pieces land in the unused buffer
            const char* in_n = reinterpret_cast<const char*>(p.in + cn * 32);
            const int sg = uu * 3;
            const int ho0 = ky == 0 ? hoff[0] : (ky == 1 ? hoff[2] : hoff[4]), ho1 = ky == 0 ? hoff[1] : (ky == 1 ? hoff[3] : hoff[5]);
            const float hm0 = ky == 0 ? hmask[0] : (ky == 1 ? hmask[2] : hmask[4]), hm1 = ky == 0 ? hmask[1] : (ky == 1 ? hmask[3] : hmask[5]);
            const int hl0 = 128 * ky * LB, hl1 = ky == 2 ? hst_last : (128 * ky + 64) * LB;
            H3_AFF(cn);
            H3_STEP(0) H3_STEP(1) H3_STEP(2)
            if (++ky == 3) { ky = 0; ++c; par ^= 1; }
        }
        __syncthreads();                    // the epilogue reuses the staging memory
        DBG_T();   /* loop end */
        if (p.dbg && t == 0 && k1 - k0 > 6) { p.dbg[blockIdx.x * 24 + 21] = clock64() - ck0; p.dbg[blockIdx.x * 24 + 22] = wall_clock64() - wk0; p.dbg[blockIdx.x * 24 + 20] = (k1 - k0) * 3; }

        // ------------------------------------------------------------ stream-K hand-off (see conv_mfma_kernel)
        constexpr int NV4 = TN * 4;
        if (k0 > 0) {
            float4* slot = reinterpret_cast<float4*>(p.sk_ws) + (size_t)lb * NV4 * NT + t;
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    slot[(size_t)(j * 4 + q) * NT] = make_float4(acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (t == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(p.sk_flags + lb, p.sk_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            DBG_T(); DBG_T();
            continue;
        }
        if (k1 < nunits) {
            int covered = k1;
            for (int nb = lb + 1; covered < nunits && nb < (int)gridDim.x; ++nb) {
                const int nu0 = (int)((long long)U * nb / gridDim.x), nu1 = (int)((long long)U * (nb + 1) / gridDim.x);
                const int span = (nu1 - nu0) < (nunits - covered) ? (nu1 - nu0) : (nunits - covered);
                if (t == 0) {
                    unsigned spins = 0;
                    while (__hip_atomic_load(p.sk_flags + nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != p.sk_epoch) {
                        __builtin_amdgcn_s_sleep(4);
                        if (++spins > (1u << 22)) { if (p.sk_err) __hip_atomic_store(p.sk_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                }
                __syncthreads();
                const float4* slot = reinterpret_cast<const float4*>(p.sk_ws) + (size_t)nb * NV4 * NT + t;
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 v = slot[(size_t)(j * 4 + q) * NT];
                        acc[j][4 * q] += v.x; acc[j][4 * q + 1] += v.y; acc[j][4 * q + 2] += v.z; acc[j][4 * q + 3] += v.w;
                    }
                covered += span;
            }
        }

        DBG_T();   /* fixup end */
        // ------------------------------------------------------------ epilogue: wave = output row, MFMA rows = columns
        float* red = smem;                 // [8][BN] + [BN]
        const int oy = oy0 + wave;
        const int vh = min(H3_TH, p.OH - oy0), vw = min(H3_TW, p.OW - ox0);
        const int cnt = vh * vw;
        float lsum[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = j * 32 + col;
            const float bv = p.bias[n];
            float sm = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ox = ox0 + (r & 3) + 8 * (r >> 2) + rbase;
                const float v = acc[j][r] + bv;
                acc[j][r] = v;
                if (oy < p.OH && ox < p.OW) {
                    if (n < p.COUT) p.out[((size_t)oy * p.OW + ox) * p.COUT + n] = v;
                    sm += v;
                }
            }
            lsum[j] = sm;
        }
        if (p.partials != nullptr) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float sm = lsum[j] + __shfl_xor(lsum[j], 32);
                if (lane < 32) red[wave * BN + j * 32 + lane] = sm;
            }
            __syncthreads();
            if (t < BN) {
                float a = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) a += red[w * BN + t];
                red[8 * BN + t] = a / (float)cnt;
            }
            __syncthreads();
            float lq[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float mu = red[8 * BN + j * 32 + col];
                float q = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ox = ox0 + (r & 3) + 8 * (r >> 2) + rbase;
                    const float d = acc[j][r] - mu;
                    if (oy < p.OH && ox < p.OW) q = fmaf(d, d, q);
                }
                lq[j] = q + __shfl_xor(q, 32);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < TN; ++j)
                if (lane < 32) red[wave * BN + j * 32 + lane] = lq[j];
            __syncthreads();
            if (t < BN) {
                float a = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) a += red[w * BN + t];
                p.partials[(size_t)tile * p.COUTp + t] = make_float2(red[8 * BN + t], a);
                if (t == 0) p.counts[tile] = cnt;
            }
        }
        __syncthreads();
        DBG_T();   /* epilogue end */
    }
    if (p.dbg && t == 0) p.dbg[blockIdx.x * 24 + 23] = dbi;
}


}  // namespace

bool conv3_halo_eligible(const ConvShape& s)
{
    return !s.transposed && s.k == 3 && s.stride == 1 && s.cin_pitch % 32 == 0 && s.cin_pitch >= 32 && s.cin_pitch <= 256 && (s.coutp == 128 || s.coutp == 64);
}
// Tile count.  edge_b (fp32 kernel): when the ragged right edge is at most 16 columns wide it is covered by ceil(OH / 16) tiles of
// 16 x 16 instead of ceil(OH / 8) tiles of 8 x 32 -- the residual layers' widths (338 ... 320) leave 2 ... 18 columns there, i.e.
// up to 9 % of the matrix work used to be spent on columns outside the image.
static void h3_tiling(int OH, int OW, bool edge_b, int* tx, int* ty, int* nb)
{
    const int r = OW % H3_TW;
    *ty = (OH + H3_TH - 1) / H3_TH;
    if (edge_b && r > 0 && r <= 16 && OW > H3_TW) { *tx = OW / H3_TW; *nb = (OH + 15) / 16; }
    else { *tx = (OW + H3_TW - 1) / H3_TW; *nb = 0; }
}
int conv3_halo_tiles(const ConvLaunch& c) { int tx, ty, nb; h3_tiling(c.OH, c.OW, c.wgt16 == nullptr, &tx, &ty, &nb); return tx * ty + nb; }      // (as launch_conv3_halo)

// FAV_H3_DBG=n: print the in-kernel timeline (prologue / K loop / stream-K fix-up / epilogue, shader clock) of the n-th launch
static void h3_debug_report(const long long* h, int grid)
{
    long long t0 = h[0];
    for (int b = 0; b < grid; ++b) t0 = std::min(t0, h[b * 24]);
    double sum[4] = {0, 0, 0, 0}, tend = 0, ck = 0, wk = 0, steps = 0; int items = 0;
    for (int b = 0; b < grid; ++b) {
        const long long* r = &h[b * 24]; const int n = (int)r[23];
        for (int i = 1; i + 4 < n + 1 && i + 4 <= 21; i += 5) {
            for (int q = 0; q < 4; ++q) sum[q] += (r[i + q + 1] - r[i + q]) * 0.01;
            ++items; tend = std::max(tend, (r[i + 4] - t0) * 0.01);
        }
        ck += r[21]; wk += r[22]; steps += r[20];
    }
    fprintf(stderr, "H3DBG grid=%d items=%d  K loop: %.0f clk/step, %.3f GHz, %.3f us/step;  per block: prologue %.2f  loop %.2f  fix-up %.2f  epilogue %.2f us;  last block ends at %.2f us\n",
            grid, items, steps ? ck / steps : 0.0, wk ? ck / (wk * 10.0) : 0.0, steps ? wk * 0.01 / steps : 0.0,
            sum[0] / grid, sum[1] / grid, sum[2] / grid, sum[3] / grid, tend);
}

template <int BN, bool S2, bool BF>
static int launch_h3_t(const H3Args& a0, int cin, int reserve_cus, bool no_sk, hipStream_t st)
{
    const auto kern = BF ? conv3_halo_bf16_kernel<BN, S2> : conv3_halo_kernel<BN, S2>;
    const size_t lds = BF ? (size_t)(2 * (H3_TH + 2) * (H3_TW + 2) * 40 + 3 * BN * 40) * 2 + (size_t)4 * cin * sizeof(float)
                          : (size_t)(2 * (H3_TH + 2) * (H3_TW + 2) * LDSS + 3 * BN * LDSS + 4 * cin) * sizeof(float);
    static PerDevice cache;
    const int dv = cur_dev();
    int cus = cache.get(dv);
    if (!cus) {
        FAV_HIP(first_launch_setup(dv, &cus, kern));
        int occ = 0;
        FAV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 512, lds));
        if (occ < 1) { set_error("halo conv: kernel does not fit on a CU"); return FAV_EHIP; }
        cache.set(dv, cus);          // one block per CU
    }
    int nres = persistent_slots(cus, reserve_cus);
    if (nres > SK_GRID) nres = SK_GRID;
    const int tiles = a0.tiles_x * a0.tiles_y + a0.nb;
    // no_sk (shared device): one block per tile -- the unit range of block b is then exactly tile b, nothing is handed between blocks
    // and nothing needs to be co-resident
    // Almost exactly one tile per CU (the 16x16 edge tiles bring six of the ten residual layers to 242 / 252 tiles for 256 CUs): one
    // whole tile per block beats stream-K there -- the 12/11.8 longer K range costs less than the second prologue and the
    // hand-off of a split tile (measured: timeline in DESIGN.md section 4)
    // (threshold swept on the MI355X: 165.1 us without, 161.3 at 96 %, 159.6 at 94 %, 159.8 at 89 %)
    const bool one_per_cu = tiles <= nres && tiles * 100 >= nres * 94;
    const int grid = (no_sk || one_per_cu) ? tiles : (tiles * (cin / 32) * 3 < nres ? 1 : nres);      // (stream-K units: tap rows)
    H3Args a = a0; a.dbg = nullptr;
    static int dbg_n = diag_env("FAV_H3_DBG") ? atoi(diag_env("FAV_H3_DBG")) : 0;
    static long long* dbuf = nullptr;
    const bool dbg = dbg_n > 0 && BN == 128 && !BF && --dbg_n == 0;
    if (dbg) { FAV_HIP(hipMalloc(reinterpret_cast<void**>(&dbuf), SK_GRID * 24 * 8)); FAV_HIP(hipMemsetAsync(dbuf, 0, SK_GRID * 24 * 8, st)); a.dbg = dbuf; }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, a);
    FAV_LAUNCH_CHECK("conv3_halo_kernel");
    if (dbg) {
        std::vector<long long> h((size_t)SK_GRID * 24);
        FAV_HIP(hipStreamSynchronize(st)); FAV_HIP(hipMemcpy(h.data(), dbuf, h.size() * 8, hipMemcpyDeviceToHost));
        h3_debug_report(h.data(), grid);
    }
    return FAV_OK;
}

int launch_conv3_halo(const ConvLaunch& c, hipStream_t st)
{
    FAV_REQUIRE(conv3_halo_eligible(conv_shape(c)) && c.KH == c.KW && !c.final_mode && !c.stuff && c.sk_ws && c.sk_flags,
                "halo conv: not eligible");
    FAV_REQUIRE((long long)((c.IH >> c.ups) + 1) * c.IWp * c.CIN < (1ll << 31), "halo conv: tensor too large for 32-bit offsets");
    H3Args a;
    a.in = c.in; a.wgt = c.wgt; a.bias = c.bias;
    a.scale1 = c.pre.scale1; a.shift1 = c.pre.shift1; a.scale2 = c.pre.scale2; a.shift2 = c.pre.shift2;
    a.stages = c.pre.stages; a.relu1 = c.pre.relu1; a.relu2 = c.pre.relu2;
    a.out = c.out; a.partials = reinterpret_cast<float2*>(c.partials); a.counts = c.counts;
    a.sk_ws = c.sk_ws; a.sk_flags = c.sk_flags; a.sk_epoch = c.sk_epoch; a.sk_err = c.sk_err;
    a.IH = c.IH; a.IW = c.IW; a.IWp = c.IWp; a.ups = c.ups; a.CIN = c.CIN; a.COUT = c.COUT; a.COUTp = c.COUTp; a.pad = c.pad;
    a.OH = c.OH; a.OW = c.OW; a.Kpad = c.Kpad;
    h3_tiling(c.OH, c.OW, c.wgt16 == nullptr, &a.tiles_x, &a.tiles_y, &a.nb);      // (the bf16 fast-mode kernel keeps 8 x 32 tiles only)
    const bool s2 = c.pre.stages >= 2;
    a.wgt16 = c.wgt16;
    if (c.wgt16) {           // fast mode: bf16 operands
        if (c.COUTp == 128) return s2 ? launch_h3_t<128, true, true>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st) : launch_h3_t<128, false, true>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st);
        return s2 ? launch_h3_t<64, true, true>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st) : launch_h3_t<64, false, true>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st);
    }
    if (c.COUTp == 128) return s2 ? launch_h3_t<128, true, false>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st) : launch_h3_t<128, false, false>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st);
    return s2 ? launch_h3_t<64, true, false>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st) : launch_h3_t<64, false, false>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st);
}

}  // namespace fav
