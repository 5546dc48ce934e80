// kernels_halo_s2.hip -- the halo-resident 3x3 stride-2 kernel (conv3s2_halo_kernel).
#include <algorithm>

#include "fav_internal.h"
#include "conv_device.h"
#include "launch_common.h"

namespace fav {

// ------------------------------------------------------------------------------------------------
// 3x3 STRIDE-2 layers (d64: 32 -> 64 at 1360x800, d128: 64 -> 128 at 680x400; models_video.lua:88-92): halo-resident implicit
// GEMM with even / odd column planes.  The generic kernel re-gathers its operand per tap with 2-5 vector-ALU instructions per
// MFMA (address arithmetic + the pending transform, nine times per element) and reaches 0.44 / 0.55 of the fp32 MFMA peak on
// these two layers.  Here a block (8 waves, one per CU, stream-K over (tile, slice, tap row) units like the stride-1 kernel)
// owns a 4 x 32 pixel output tile: wave = (output row, half of the output channels).  Per 32-channel slice the
// (2*4+1) x (2*32+1) = 9 x 65 pixel halo is gathered ONCE (IN/ReLU applied, zero padding) into LDS as two planes -- even
// input columns (33 per row) and odd input columns (32 per row) -- so that for every tap the 32 lanes of a wave (32 consecutive
// OUTPUT columns = input columns 2m + kx) read 32 CONSECUTIVE pixels of one plane: conflict-free ds_read_b128, immediate tap
// offsets.  585 pixels x 144 B = 84 KB: one halo buffer only, so the next slice's halo travels through registers (10 pieces of
// 16 bytes per thread, loaded one per K step) and is written between slices.  Weights stream through the same 3-slot ring as
// in the stride-1 kernel; one barrier per K step (mid-step), two per slice change.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int S2_TH = 4, S2_TW = 32;                 // output tile
constexpr int S2_HR = 2 * S2_TH + 1;                 // 9 halo rows
constexpr int S2_EW = S2_TW + 1, S2_OW = S2_TW;      // even / odd plane widths (33, 32)
constexpr int S2_EP = S2_HR * S2_EW;                 // 297 pixels in the even plane
constexpr int S2_HP = S2_EP + S2_HR * S2_OW;         // 585 halo pixels
constexpr int S2_NHV = 10;                           // 16-byte halo pieces per thread and slice (585 * 8 / 512 = 9.14)

struct S2Args {
    const float* in; const float* wgt; const float* bias;
    const float* scale1; const float* shift1;
    float* out; float2* partials; int* counts;
    float* sk_ws; unsigned* sk_flags; unsigned sk_epoch; unsigned* sk_err;
    int IH, IW, IWp, CIN, COUT, COUTp, pad, OH, OW, Kpad, tiles_x, tiles_y;
    int stages, relu1;
};

template <int BN>
__global__ __launch_bounds__(512, 2) void conv3s2_halo_kernel(const S2Args p)
{
    constexpr int NT = 512;
    constexpr int TN = BN / 64;                       // 32-channel accumulator tiles per wave (a wave owns BN/2 channels)
    constexpr int BROWS = BN / 64;                    // weight rows per thread per step
    constexpr int ALIAS = NT * S2_NHV - S2_HP * 8;    // staging units past the end alias earlier ones (same data, same slot)
    static_assert(ALIAS % 8 == 0 && ALIAS >= 0 && ALIAS <= NT, "halo aliasing");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Hs = smem;                                 // [585][LDSS]: even plane, then odd plane
    float* Bs = Hs + S2_HP * LDSS;                    // [3][BN][LDSS]
    float* aff = Bs + 3 * BN * LDSS;                  // [2][CIN]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave & 3, nh = wave >> 2;          // output row of the tile, channel half
    const int CIN = p.CIN;
    const int nchunks = CIN >> 5, nsteps = nchunks * 9;
    const int ntiles = p.tiles_x * p.tiles_y;
    const int lb = xcd_linear_block();
    for (int i = t; i < CIN; i += NT) { aff[i] = p.stages >= 1 ? p.scale1[i] : 1.f; aff[CIN + i] = p.stages >= 1 ? p.shift1[i] : 0.f; }
    const float lo1 = (p.stages >= 1 && p.relu1) ? 0.f : -INFINITY;

    const int c4 = t & 7, r0 = t >> 3;
    const int frag_k = (lane >> 5) * 4, m = lane & 31;
    const int col = lane & 31, rbase = 4 * (lane >> 5);
    const unsigned wofs = (unsigned)(r0 * p.Kpad + c4 * 4) * 4u;
    const unsigned wrow64 = (unsigned)(64 * p.Kpad) * 4u;
    float* const bst = Bs + r0 * LDSS + c4 * 4;                                        // weight staging slot (ring slot 0)
    // A fragments: even plane (kx = 0, 2) and odd plane (kx = 1), tap row 0, this wave's output row
    const float* const afrE = Hs + ((2 * wr) * S2_EW + m) * LDSS + frag_k;
    const float* const afrO = Hs + (S2_EP + (2 * wr) * S2_OW + m) * LDSS + frag_k;
    const float* const bfr = Bs + (nh * (BN / 2) + m) * LDSS + frag_k;                 // B fragments: ring slot 0, this wave's channels
    const float* const affr = aff + c4 * 4;

    // halo piece i of this thread: staging unit e = t + 512 i -> halo pixel e >> 3 (plane-major), 16-byte chunk c4.  Its position
    // inside the halo is fixed; the tile only moves the origin.
    int hlds[S2_NHV], hyx[S2_NHV];
#pragma unroll
    for (int i = 0; i < S2_NHV; ++i) {
        int e = t + NT * i; e -= e >= S2_HP * 8 ? ALIAS : 0;
        const int pe = e >> 3;
        int hy, hx;
        if (pe < S2_EP) { hy = pe / S2_EW; hx = 2 * (pe - hy * S2_EW); }
        else { const int q = pe - S2_EP; hy = q / S2_OW; hx = 2 * (q - hy * S2_OW) + 1; }
        hlds[i] = pe * LDSS + c4 * 4;
        hyx[i] = hy << 16 | hx;
    }

    // Work of this block: a contiguous range of stream-K units (unit = one tap row = 3 K steps of one slice of one tile), walked
    // as SEGMENTS = the part of one (tile, slice) inside the range.  While a segment computes, the halo of the NEXT segment --
    // the next slice of the tile or the first slice of the next tile -- is fetched into registers (hq), so that neither a slice
    // change nor a tile change waits for memory: these layers read 1.1 x their input once per tile and are otherwise
    // bandwidth-exposed (d64: 229 MB of traffic against 72 us of matrix work).
    const int nunits = nchunks * 3;
    const int U = ntiles * nunits;
    int u = (int)((long long)U * lb / gridDim.x);
    const int u_end = (int)((long long)U * (lb + 1) / gridDim.x);

    int hoff[S2_NHV]; float hmask[S2_NHV];            // of the segment being FETCHED
    float4 hq[S2_NHV];
    v4f rb[BROWS];
#define S2_TILE_SETUP(tile_)                                                                        \
    {   const int ty_ = (tile_) / p.tiles_x, tx_ = (tile_) - ty_ * p.tiles_x;                       \
        _Pragma("unroll") for (int i = 0; i < S2_NHV; ++i) {                                        \
            const int iy = 2 * ty_ * S2_TH - p.pad + (hyx[i] >> 16), ix = 2 * tx_ * S2_TW - p.pad + (hyx[i] & 0xffff); \
            const bool v = ((unsigned)iy < (unsigned)p.IH) & ((unsigned)ix < (unsigned)p.IW);       \
            hoff[i] = ((v ? (iy * p.IWp + ix) * CIN : 0) + c4 * 4) * 4;                             \
            hmask[i] = v ? 1.f : 0.f;                                                               \
        } }
#define S2_XFORM(v_, sc_, sh_, m_)                                                                  \
    { v_.x = fmaxf(fmaf(v_.x, sc_.x, sh_.x), lo1) * m_; v_.y = fmaxf(fmaf(v_.y, sc_.y, sh_.y), lo1) * m_;  \
      v_.z = fmaxf(fmaf(v_.z, sc_.z, sh_.z), lo1) * m_; v_.w = fmaxf(fmaf(v_.w, sc_.w, sh_.w), lo1) * m_; }
// parked pieces (slice cs_) -> transformed -> the halo buffer
#define S2_COMMIT(cs_)                                                                              \
    {   const v4f sc_ = *reinterpret_cast<const v4f*>(affr + (cs_) * 32), sh_ = *reinterpret_cast<const v4f*>(affr + CIN + (cs_) * 32); \
        _Pragma("unroll") for (int i = 0; i < S2_NHV; ++i) { S2_XFORM(hq[i], sc_, sh_, hmask[i]); *reinterpret_cast<float4*>(Hs + hlds[i]) = hq[i]; } }
#define S2_LOAD_B(gs_)                                                                              \
    { const float* src_ = p.wgt + min((gs_), nsteps - 1) * BK;                                      \
      _Pragma("unroll") for (int j = 0; j < BROWS; ++j) rb[j] = *reinterpret_cast<const v4f*>(reinterpret_cast<const char*>(src_) + (wofs + j * wrow64)); }
#define S2_STORE_B(slot_)                                                                           \
    { _Pragma("unroll") for (int j = 0; j < BROWS; ++j) *reinterpret_cast<v4f*>(bst + ((slot_) * BN + 64 * j) * LDSS) = rb[j]; }

    // first segment of the range: fetched with exposed latency, once per block
    int tile = 0, c = 0, t_lo = 0, t_hi = 0;          // current segment: slice c of `tile`, taps [t_lo, t_hi)
    int k1 = 0;                                       // end (in units) of the current work item inside its tile
    if (u < u_end) {
        tile = u / nunits;
        const int k0 = u - tile * nunits;
        k1 = (u_end - u) < nunits - k0 ? k0 + (u_end - u) : nunits;
        c = (k0 * 21846) >> 16; t_lo = 3 * (k0 - c * 3);
        t_hi = min(9, 3 * (k1 - c * 3));
        S2_TILE_SETUP(tile);
        const char* in0 = reinterpret_cast<const char*>(p.in + c * 32);
#pragma unroll
        for (int i = 0; i < S2_NHV; ++i) hq[i] = *reinterpret_cast<const float4*>(in0 + hoff[i]);
        S2_LOAD_B(c * 9 + t_lo);
        __syncthreads();                              // transform tables
        S2_COMMIT(c);
        S2_STORE_B(0);
        S2_LOAD_B(c * 9 + t_lo + 1);
    }
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    bool item_start = true;                           // the current segment opens a work item (its tile's accumulators start at 0)
    int k0_item = u < u_end ? u - tile * nunits : 0;  // first unit of the current work item inside its tile
    __syncthreads();

    v4f fa[2], fb[2][TN];
#define S2_FRAG(set_, ap_, bp_)                                                                     \
    { fa[set_] = *reinterpret_cast<const v4f*>(ap_);                                                \
      _Pragma("unroll") for (int j = 0; j < TN; ++j) fb[set_][j] = *reinterpret_cast<const v4f*>((bp_) + j * 32 * LDSS); }
#define S2_MFMA(set_)                                                                               \
    { _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                              \
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_].x, fb[set_][j].x, acc[j], 0, 0, 0);  \
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_].y, fb[set_][j].y, acc[j], 0, 0, 0);  \
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_].z, fb[set_][j].z, acc[j], 0, 0, 0);  \
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_].w, fb[set_][j].w, acc[j], 0, 0, 0); } }
// A-fragment base of tap T_ (compile time): even plane for kx = 0 / 2 (shifted by one pixel), odd plane for kx = 1
#define S2_ABASE(T_) (((T_) % 3 == 1 ? afrO + ((T_) / 3) * S2_OW * LDSS : afrE + (((T_) / 3) * S2_EW + ((T_) % 3 == 2 ? 1 : 0)) * LDSS))
// one K step = tap T_ of the current slice (32 channels); ring slot = T_ % 3.  The weights two steps ahead in EXECUTION order are
// requested (the step after the segment's last one is the first step of the next segment: ngs), and piece T_ of the next
// segment's halo (piece 9 rides with tap 0).  PIN_: the group-0 fragments were read by the previous step; POUT_: read those of
// tap T_ + 1 (compile time: a run-time flag here costs dozens of v_mov per step).
#define S2_STEP(T_, PIN_, POUT_)                                                                    \
    {                                                                                               \
        const float* a_ = S2_ABASE(T_);                                                             \
        const float* b_ = bfr + ((T_) % 3) * BN * LDSS;                                             \
        if (!(PIN_)) S2_FRAG(0, a_, b_);                                                            \
        S2_FRAG(1, a_ + 8, b_ + 8);                                                                 \
        S2_STORE_B(((T_) + 1) % 3);                                                                 \
        S2_LOAD_B((T_) + 2 < t_hi ? c * 9 + (T_) + 2 : ngs + ((T_) + 2 - t_hi));                    \
        if (has_next) { hq[T_] = *reinterpret_cast<const float4*>(in_n + hoff[T_]); if ((T_) == 0) hq[9] = *reinterpret_cast<const float4*>(in_n + hoff[9]); } \
        S2_MFMA(0);                                                                                 \
        S2_FRAG(0, a_ + 16, b_ + 16); S2_MFMA(1);                                                   \
        __syncthreads();                                                                            \
        S2_FRAG(1, a_ + 24, b_ + 24); S2_MFMA(0);                                                   \
        if (POUT_) { constexpr int TNX = ((T_) + 1) % 9; S2_FRAG(0, S2_ABASE(TNX), bfr + (TNX % 3) * BN * LDSS); } \
        S2_MFMA(1);                                                                                 \
    }
#define S2_STEP_IF(T_) if ((T_) >= t_lo && (T_) < t_hi) S2_STEP(T_, false, false)

    while (u < u_end) {
        // ---- the segment after this one
        const int seg_units = (t_hi - t_lo) / 3;
        const bool item_end = (c * 3 + t_hi / 3) == k1;             // this segment closes the work item (end of the tile or of the range)
        int n_tile = tile, n_c = c + 1, n_lo = 0, n_hi = 9, n_k1 = k1;
        const int u_next = u + seg_units;
        const bool has_next = u_next < u_end;
        if (item_end) {                                             // next segment = head of the next tile
            n_tile = tile + 1; n_c = 0; n_lo = 0;
            n_k1 = (u_end - u_next) < nunits ? (u_end - u_next) : nunits;
        }
        n_hi = min(9, 3 * (n_k1 - n_c * 3));
        const int ngs = has_next ? n_c * 9 + n_lo : nsteps - 1;
        const char* in_n = reinterpret_cast<const char*>(p.in + n_c * 32);
        if (has_next) {
            if (item_end) S2_TILE_SETUP(n_tile);                    // (hoff / hmask now describe the segment being fetched)
            // pieces whose step this (partial) segment does not execute
#pragma unroll
            for (int i = 0; i < S2_NHV; ++i) if (!(i >= t_lo && i < t_hi) && !(i == 9 && t_lo == 0)) hq[i] = *reinterpret_cast<const float4*>(in_n + hoff[i]);
        }
        if (t_lo == 0 && t_hi == 9) {
            // whole slice (the common case): fragments of the next tap are read one step ahead
            S2_STEP(0, false, true) S2_STEP(1, true, true) S2_STEP(2, true, true) S2_STEP(3, true, true) S2_STEP(4, true, true)
            S2_STEP(5, true, true) S2_STEP(6, true, true) S2_STEP(7, true, true) S2_STEP(8, true, false)
        } else {
            // a split tile's partial slice: plain steps
            S2_STEP_IF(0) S2_STEP_IF(1) S2_STEP_IF(2) S2_STEP_IF(3) S2_STEP_IF(4) S2_STEP_IF(5) S2_STEP_IF(6) S2_STEP_IF(7) S2_STEP_IF(8)
        }
        u = u_next;

        if (item_end) {
            __syncthreads();                    // everybody is done with the halo: the epilogue reuses the start of the staging memory
            const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
            const int oy0 = ty * S2_TH, ox0 = tx * S2_TW;
            // ------------------------------------------------------------ stream-K hand-off (as in conv3_halo_kernel)
            constexpr int NV4 = TN * 4;
            bool owner = true;
            if (k0_item > 0) {
                owner = false;
                float4* slot = reinterpret_cast<float4*>(p.sk_ws) + (size_t)lb * NV4 * NT + t;
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        store16_wt(slot + (size_t)(j * 4 + q) * NT, v4f{acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]});
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (t == 0) __hip_atomic_store(p.sk_flags + lb, p.sk_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (k1 < nunits) {
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
            if (owner) {
                // -------------------------------------------------------- epilogue: wave = (output row, channel half), MFMA rows = columns
                float* red = smem;                 // [8 waves][BN/2] float2 + [8] int
                const int oy = oy0 + wr;
                float lsum[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = nh * (BN / 2) + j * 32 + col;
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
                    float2* st = reinterpret_cast<float2*>(red);      // [4 rows][BN]: the two channel halves of a row sit side by side
                    int* wn = reinterpret_cast<int*>(red + 2 * S2_TH * BN);
                    const int nw = oy < p.OH ? min(S2_TW, p.OW - ox0) : 0;
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const float sm = lsum[j] + __shfl_xor(lsum[j], 32);
                        const float mu = nw ? sm / (float)nw : 0.f;
                        float q = 0.f;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int ox = ox0 + (r & 3) + 8 * (r >> 2) + rbase;
                            const float d = acc[j][r] - mu;
                            if (oy < p.OH && ox < p.OW) q = fmaf(d, d, q);
                        }
                        q += __shfl_xor(q, 32);
                        if (lane < 32) st[wr * BN + nh * (BN / 2) + j * 32 + lane] = make_float2(mu, q);
                    }
                    if (lane == 0 && nh == 0) wn[wr] = nw;
                    __syncthreads();
                    if (t < BN) {
                        int n;
                        p.partials[(size_t)tile * p.COUTp + t] = merge_wave_stats(st, wn, S2_TH, BN, t, &n);
                        if (t == 0) p.counts[tile] = n;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            k0_item = 0;
        }
        if (has_next) {
            // segment change: the parked pieces (transformed) replace the halo
            __syncthreads();
            S2_COMMIT(n_c);
            __syncthreads();
        }
        tile = n_tile; c = n_c; t_lo = n_lo; t_hi = n_hi; k1 = n_k1;
        (void)item_start;
    }
}

}  // namespace

bool conv3s2_eligible(const ConvShape& s)
{
    // 64 output channels only: the 128-wide instance (d128) measured 126 us against 115 us of the generic kernel (register
    // pressure: accumulators + the parked halo), the 64-wide one 122 us against 148 us (d64)
    return !s.transposed && s.k == 3 && s.stride == 2 && s.ups == 0 && s.stages <= 1 && s.cin_pitch % 32 == 0 && s.cin_pitch >= 32 && s.cin_pitch <= 256 && s.coutp == 64;
}
int conv3s2_tiles(const ConvLaunch& c) { return ((c.OH + S2_TH - 1) / S2_TH) * ((c.OW + S2_TW - 1) / S2_TW); }

template <int BN>
static int launch_s2_t(const S2Args& a, int cin, int reserve_cus, bool no_sk, hipStream_t st)
{
    const auto kern = conv3s2_halo_kernel<BN>;
    const size_t lds = (size_t)(S2_HP * LDSS + 3 * BN * LDSS + 2 * cin) * sizeof(float);
    static PerDevice cache;
    const int dv = cur_dev();
    int cus = cache.get(dv);
    if (!cus) {
        FAV_HIP(first_launch_setup(dv, &cus, kern));
        int occ = 0;
        FAV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 512, lds));
        if (occ < 1) { set_error("stride-2 halo conv: kernel does not fit on a CU"); return FAV_EHIP; }
        cache.set(dv, cus);
    }
    int nres = persistent_slots(cus, reserve_cus);
    if (nres > SK_GRID) nres = SK_GRID;
    const int tiles = a.tiles_x * a.tiles_y;
    const int grid = no_sk ? tiles : (tiles * (cin / 32) * 3 < nres ? 1 : nres);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, a);
    FAV_LAUNCH_CHECK("conv3s2_halo_kernel");
    return FAV_OK;
}

int launch_conv3s2(const ConvLaunch& c, hipStream_t st)
{
    FAV_REQUIRE(conv3s2_eligible(conv_shape(c)) && c.KH == c.KW && !c.final_mode && !c.stuff && c.sk_ws && c.sk_flags,
                "stride-2 halo conv: not eligible");
    FAV_REQUIRE((long long)(c.IH + 1) * c.IWp * c.CIN < (1ll << 31), "stride-2 halo conv: tensor too large for 32-bit offsets");
    S2Args a;
    a.in = c.in; a.wgt = c.wgt; a.bias = c.bias; a.scale1 = c.pre.scale1; a.shift1 = c.pre.shift1; a.stages = c.pre.stages; a.relu1 = c.pre.relu1;
    a.out = c.out; a.partials = reinterpret_cast<float2*>(c.partials); a.counts = c.counts;
    a.sk_ws = c.sk_ws; a.sk_flags = c.sk_flags; a.sk_epoch = c.sk_epoch; a.sk_err = c.sk_err;
    a.IH = c.IH; a.IW = c.IW; a.IWp = c.IWp; a.CIN = c.CIN; a.COUT = c.COUT; a.COUTp = c.COUTp; a.pad = c.pad;
    a.OH = c.OH; a.OW = c.OW; a.Kpad = c.Kpad;
    a.tiles_x = (c.OW + S2_TW - 1) / S2_TW; a.tiles_y = (c.OH + S2_TH - 1) / S2_TH;
    return launch_s2_t<64>(a, c.CIN, c.reserve_cus, c.no_sk != 0, st);
}

}  // namespace fav
