// Internal declarations shared by the libfav translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "../../include/fav.h"

// Environment variables.  A RELEASE build of the library (the default `make`: libfav.so) reads only the documented ones -- FAV_SIDE_CUS,
// FAV_SIDE_QUEUES, FAV_ROCTX in the library; FAV_GPU, FAV_CC_*, FAV_RCCL_TIMEOUT_S, FAV_TEST_WORKER_FAIL in the executables.  Every
// kernel-selection, tuning and debug switch (FAV_NO_*, FAV_WINO_F2, FAV_W4_*, FAV_*_DBG, ...) goes through diag_env() and exists in the
// DIAGNOSTIC build only (`make diag`: libfav_diag.so, -DFAV_DIAG; what the cross-check tests and the A/B scripts load): a stray FAV_NO_WINO
// in a user's environment cannot silently halve the rate of the library that ships.
#include <cstdlib>
inline const char* diag_env(const char* name)
{
#ifdef FAV_DIAG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

namespace fav {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define FAV_HIP(expr)                                              \
    do {                                                           \
        hipError_t e__ = (expr);                                   \
        if (e__ != hipSuccess) return ::fav::hip_fail(e__, #expr); \
    } while (0)
#define FAV_LAUNCH_CHECK(name)                                            \
    do {                                                                  \
        hipError_t e__ = hipGetLastError();                               \
        if (e__ != hipSuccess) return ::fav::hip_fail(e__, "launch " name); \
    } while (0)
#define FAV_REQUIRE(cond, ...)                 \
    do {                                       \
        if (!(cond)) {                         \
            ::fav::set_error(__VA_ARGS__);     \
            return FAV_EINVAL;                 \
        }                                      \
    } while (0)

// No exception may cross the C ABI (include/fav.h): entry points that parse untrusted files run their body inside this pair.
#define FAV_ABI_TRY try {
#define FAV_ABI_CATCH(where_)                                                                                            \
    } catch (const std::bad_alloc&) {                                                                                   \
        ::fav::set_error(where_ ": out of memory while parsing (damaged size field?)"); return FAV_EFORMAT;                \
    } catch (const std::exception& e__) {                                                                               \
        ::fav::set_error(where_ ": %s", e__.what()); return FAV_EFORMAT;                                                  \
    } catch (...) {                                                                                                     \
        ::fav::set_error(where_ ": unexpected exception"); return FAV_EFORMAT;                                            \
    }

int ensure_device();   // FAV_OK or FAV_ENODEVICE

// roctx ranges around the stages of a frame (mask / certainty + input assembly / network, and every convolution inside it) for
// rocprofv3 --marker-trace.  Off unless FAV_ROCTX=1: the marker library is then dlopen'ed (libfav itself does not link it).
struct TraceRange {
    explicit TraceRange(const char* name);
    ~TraceRange();
    static bool enabled();
    bool on;
};

// ------------------------------------------------------------------------------------------------
// host-side description of a parsed checkpoint (t7_reader.cpp)
// ------------------------------------------------------------------------------------------------
enum LayerType { L_PAD, L_CONV, L_IN, L_RELU, L_RES, L_UP, L_TANH, L_MUL, L_IDENTITY, L_BN };

struct Layer {
    LayerType type = L_IDENTITY;
    // pad: nn.SpatialReflectionPadding (pad_mode 0) / nn.SpatialReplicationPadding (pad_mode 1), models_video.lua:12-16,27-31,70-77
    int pl = 0, pr = 0, pt = 0, pb = 0, pad_mode = 0;
    // conv
    int cin = 0, cout = 0, k = 0, stride = 1, pad = 0;
    int transposed = 0, adj = 0;    // nn.SpatialFullConvolution: w is [cin][cout][k][k]
    std::vector<float> w, b;        // [cout][cin][k][k], [cout] (may be empty)
    // instance norm / batch norm (evaluate mode: running mean / var)
    std::vector<float> gamma, beta, mean, var;
    float eps = 1e-5f;
    // upsample / mul / shave
    int scale = 1;
    float mul = 1.f;
    int shave = 0;
    std::vector<Layer> block;       // residual branch
    int dev_index = -1;             // executed copy only: this layer's entry in fav_net::convs (conv) | ins (instance / batch norm), set by upload_layers
};

int t7_parse_model(const char* path, std::vector<Layer>& out);          // .t7 -> layer list
int blob_pack(const std::vector<Layer>& layers, std::vector<uint8_t>& blob);
int blob_unpack(const void* blob, size_t bytes, std::vector<Layer>& out);
std::string describe_layers(const std::vector<Layer>& layers, int indent = 0);

// ------------------------------------------------------------------------------------------------
// device kernels: launch wrappers (each enqueues on `st` and does not synchronise)
// ------------------------------------------------------------------------------------------------
struct Affine {            // pending per-channel transform t(x) = relu?(x*scale+shift), up to two stages
    const float* scale1 = nullptr; const float* shift1 = nullptr; int relu1 = 0;
    const float* scale2 = nullptr; const float* shift2 = nullptr; int relu2 = 0;
    int stages = 0;
    // Round 5: stage 1 as an InstanceNorm whose statistics are still ACCUMULATORS (stat_acc.h): the producing convolution added every
    // work unit's exact fixed-point (sum, sum of squares) to them with integer atomics, the CONSUMER forms scale / shift in its
    // prologue (no in_finalize launch in between).  acc1 != null => scale1 / shift1 are null; only conv3_wino4_kernel<1> takes it
    const long long* acc1 = nullptr; long long* acc1_zero = nullptr;      // this frame's accumulators | the other parity's (zeroed by the consumer for the next frame)
    const float* gamma1 = nullptr; const float* beta1 = nullptr; float eps1 = 0.f; int count1 = 0;
};
// accumulator layout of one InstanceNorm: [parity 2][copy STAT_COPIES][channel C][4 words: sum lo, sum hi, squares lo, squares hi]
constexpr int STAT_COPIES = 8;       // one copy per XCD (blockIdx & 7): 8x shallower chains of atomics on one address
inline size_t stat_acc_words(int C) { return (size_t)STAT_COPIES * C * 4; }      // per parity
// A unit whose statistics are not finite (a diverged clip, a damaged checkpoint: NaN / Inf activations) cannot be written as fixed point
// (the double -> integer conversion would be undefined): its producer adds STAT_NONFINITE to the HIGH words instead, and a consumer that
// finds a high word beyond STAT_NONFINITE / 2 in magnitude forms NaN scale / shift -- what in_finalize_kernel gives for the same input.
// What the two words carry: a high word counts 2^-8 (value * 2^40 = hi * 2^32 + lo), and a channel's high words, summed over all its
// units, must stay below STAT_NONFINITE / 2 = 2^52 in magnitude.  A producer therefore takes a unit's term v (n mean, or M2 + n mean^2 of
// at most 16 x 16 pixels) as finite only while |hi| x (units per channel) < STAT_UNIT_HI_SUM = 2^51 -- the floor of a negative term adds at
// most one per unit, far less than the other 2^51 -- and poisons the channel beyond that (NaN, not a wrong value).  In activations:
//   a frame of U units carries a unit mean square below 2^43 / (256 U): RMS < 2^13.5 = 11 900 at 320 x 180 (1280 x 720 frames, U = 240),
//   < 2^12 = 4 100 at 960 x 540 (3840 x 2160, U = 2 040), < 2^10.5 = 1 448 at the 2^22 pixels (U = 2^14) launch_conv3_wino4 stops at.
// The partials form (in_finalize_kernel, fp64) has no such limit.  The poison itself: k non-finite units add k x 2^53, which leaves 64
// bits from k = 2^10 on; the wrapped sum is still beyond 2^52 in magnitude unless k is a multiple of 2 048, so frames of fewer than
// 2 048 units (up to 3840 x 2160) cannot lose it.
constexpr long long STAT_NONFINITE = 1ll << 53;
constexpr double STAT_UNIT_HI_SUM = 2251799813685248.0;      // 2^51
__host__ __device__ inline bool stat_acc_poisoned(long long hi_sum, long long hi_squares)
{
    return hi_sum >= STAT_NONFINITE / 2 || hi_sum <= -(STAT_NONFINITE / 2) || hi_squares >= STAT_NONFINITE / 2 || hi_squares <= -(STAT_NONFINITE / 2);
}

struct ConvLaunch {
    const float* in = nullptr;      // NHWC physical [IHp][IWp][CIN]
    int IH = 0, IW = 0;             // logical input size (after `ups` nearest upsampling)
    int IWp = 0;                    // physical row pitch in pixels
    int ups = 0;                    // log2 of the nearest-upsample factor applied on load (0|1)
    int stuff = 0;                  // with ups=1: zero-stuffed instead of replicated (transposed convolution as a convolution)
    int CIN = 0;                    // physical channels (multiple of 4)
    Affine pre;                     // applied on load (zero padding is applied AFTER it)
    const float* wgt = nullptr;     // [COUTp][Kpad], k = tap*CIN + ci
    const unsigned short* wgt16 = nullptr;   // bf16 copy of wgt: selects the bf16-operand halo kernel (fast mode) when set
    const float* bias = nullptr;    // [COUTp]
    int COUT = 0, COUTp = 0;        // valid / padded (multiple of the N tile) output channels
    int KH = 0, KW = 0, stride = 1, pad = 0;
    int Kpad = 0;                   // multiple of 32
    int OH = 0, OW = 0;
    float* out = nullptr;           // NHWC [OH][OW][COUT]   (mode 0)
    float* partials = nullptr;      // [mblocks][COUTp] float2 (mean, M2) or null
    // final-layer epilogue (mode 1): out_planar[2-c][m] = (tanh(v)*tanh_mul + mean[c]) / 255
    int final_mode = 0;
    float tanh_mul = 1.f;
    float* out_planar = nullptr;    // [3][OH][OW] RGB  (deprocessed)   or null
    float* out_raw_nchw = nullptr;  // [3][OH][OW] BGR  (150*tanh)      or null
    // stream-K hand-off state (conv_streamk_workspace_bytes() floats, conv_streamk_grid() flags, a launch-unique
    // epoch > 0); null => plain data-parallel launch
    float* sk_ws = nullptr; unsigned* sk_flags = nullptr; unsigned sk_epoch = 0;
    unsigned* sk_err = nullptr;     // host-mapped error word (device pointer): set by a hand-off wait that timed out
    int reserve_cus = 0;            // CUs left to concurrent side-queue work: persistent / stream-K grids shrink by this many
    int no_sk = 0;                  // shared device: data-parallel grids only (no hand-off between blocks, no co-residency assumption)
    // Winograd kernel only.  A pending residual join as the input: in = the branch's raw output y (one pending InstanceNorm, no ReLU),
    // join_skip = the skip tensor's pixel under y's pixel (0, 0) at the SAME row pitch IWp, join_out = where the joined tensor is
    // written (pitch IWp as well).  OWp > 0: row pitch of `out` in pixels (the output is laid out under a later join's skip tensor).
    const float* join_skip = nullptr; float* join_out = nullptr; int OWp = 0;
    // F(4x4) Winograd kernel only: accumulators of the InstanceNorm that follows (this frame's parity) instead of `partials`, or null
    long long* stat_acc = nullptr;
    // F(4x4) Winograd kernel only: meeting places of the two parts of a unit that a stream-K share boundary cuts (conv3_wino4_ksplit_bytes()
    // bytes: 256 boundaries x 2 parts x 16 x 16 pixels x 128 channels) and their arrival counters (256 ints, zero between launches);
    // null => whole units only
    float* ks_ws = nullptr; int* ks_cnt = nullptr;
    const float* wpk = nullptr;     // the selected kernel's own packing of the weights (the kernels that do not read wgt / wgt16)
    int cin_real = 0; int* counts = nullptr;      // input channels that carry data (first layer: 7 | 3 of its 8) | per-partial pixel counts, where the kernel writes them
};
// What a kernel's eligibility depends on: fav_net builds one per layer and asks every predicate below with it.  stages / ups = the pending
// normalisations and x`2^ups` upsampling of the input -- as it then is (select_conv), or as the kernel is built for (packing); a launcher checks its own descriptor
struct ConvShape { int cin_pitch = 0, cin_real = 0, cout = 0, coutp = 0, k = 0, stride = 1, pad = 0, adj = 0, transposed = 0, stages = 0, ups = 0; };
inline ConvShape conv_shape(const ConvLaunch& c, int transposed = 0, int adj = 0) { return {c.CIN, c.cin_real, c.COUT, c.COUTp, c.KH, c.stride, c.pad, adj, transposed, c.pre.stages, c.ups}; }
inline size_t conv3_wino4_ksplit_bytes() { return (size_t)256 * 2 * 256 * 128 * sizeof(float); }
// kernels_conv.hip: the generic implicit-GEMM kernel (data-parallel or stream-K)
size_t conv_streamk_workspace_bytes();
int conv_streamk_grid();
constexpr int CONV_BM = 128;
inline int conv_tiles(const ConvLaunch& p) { return (p.OH * p.OW + CONV_BM - 1) / CONV_BM; }
int launch_conv(const ConvLaunch& p, hipStream_t st);
// first layer (8-channel input pitch, 9x9), kernels_c8.hip: LDS-resident halo + weights, persistent blocks; partial statistics are
// per 16x16 tile with explicit counts
bool conv_c8_eligible(const ConvShape& s);
int conv_c8_tiles(const ConvLaunch& p);
int launch_conv_c8(const ConvLaunch& p, hipStream_t st);
// the same layer with dense K for 7 (video model) or 3 (image model) real input channels: taps paired so that no zero channel is
// multiplied; wc8d = conv_c8d_pack() of the [cout][cin][9][9] weights
bool conv_c8d_eligible(const ConvShape& s);
void conv_c8d_pack(const float* w, int cin, int cout, std::vector<float>& out);
int launch_conv_c8d(const ConvLaunch& p, hipStream_t st);
// 3x3 stride-1 layers, kernels_halo.hip: halo-resident implicit GEMM (stream-K, needs the ConvLaunch sk_* fields); partials per 8x32 tile
bool conv3_halo_eligible(const ConvShape& s);
int conv3_halo_tiles(const ConvLaunch& p);      // (no wgt16, i.e. the fp32 kernel: 16 x 16 tiles on a narrow ragged right edge)
int launch_conv3_halo(const ConvLaunch& p, hipStream_t st);
// 3x3 stride-2 layers, kernels_halo_s2.hip: halo-resident implicit GEMM with even / odd column planes (stream-K); partials per 4x32 tile
bool conv3s2_eligible(const ConvShape& s);
int conv3s2_tiles(const ConvLaunch& p);
int launch_conv3s2(const ConvLaunch& p, hipStream_t st);
// last layer with few output channels: kx taps folded into N (kernels_fold.hip); wfold = [KH][32][CIN]
bool conv_fold_eligible(const ConvShape& s);
bool conv_fold_launchable(int cin_pitch, int k, int pad, int ups, int IH, int IW);      // 128 / 256 input channels: on a x2-upsampled input only
int launch_conv_fold(const ConvLaunch& p, hipStream_t st);
// the same first layer with 1-D minimal filtering F(2,3) along x (kernels_first.hip); wpk = conv_first_pack() (first_pack.h);
// eligibility as conv_c8d_eligible; partials per 8x64 tile with explicit counts
int conv_first_tiles(const ConvLaunch& p);
int launch_conv_first(const ConvLaunch& p, hipStream_t st);
// ... and with 2-D minimal filtering F(2x2,3x3) over its nine 3x3 blocks (conv_first2d_kernel); wpk = conv_first2d_pack() (first2d_pack.h);
// partials per 16x32-pixel tile
bool conv_first2d_eligible(const ConvShape& s);      // any number of 32-filter groups
int conv_first2d_tiles(const ConvLaunch& p);
int launch_conv_first2d(const ConvLaunch& p, hipStream_t st);
// 3x3 stride-1 UNPADDED 128-channel layers (the residual blocks): Winograd F(2x2,3x3), kernels_wino.hip; wpk = conv_wino_pack()
// of the [cout][cin][3][3] weights (wino_pack.h); partials per 8x16-pixel unit with explicit counts
bool conv3_wino_eligible(const ConvShape& s);
int conv3_wino_tiles(const ConvLaunch& p);
int launch_conv3_wino(const ConvLaunch& p, hipStream_t st);
// the same layers as Winograd F(4x4,3x3), kernels_wino4.hip (round 4); wpk = conv_wino4_pack() (wino4_pack.h); partials per 16x16-pixel unit
bool conv3_wino4_eligible(const ConvShape& s);
int conv3_wino4_tiles(const ConvLaunch& p);
int launch_conv3_wino4(const ConvLaunch& p, hipStream_t st);
// 3x3 stride-1 pad-1 64-channel layer on a x2 nearest-upsampled materialised input (U2 + c3s1-64): four 2x2 convolutions on the
// physical pixels with merged weights, kernels_up2.hip; wpk = conv_up2_pack() (up2_pack.h); partials per 8x32 physical-pixel tile
bool conv3_up2_eligible(const ConvShape& s);
int conv3_up2_tiles(const ConvLaunch& p);
int launch_conv3_up2(const ConvLaunch& p, hipStream_t st);
// the 3x3 stride-2 layers (d64 / d128) with fragment-order weights read global -> registers, halo chunks of 16 channels double-buffered
// in LDS, whole tiles per block (kernels_s2.hip); wpk = conv_s2w_pack() (s2_pack.h); partials per TR x 32 output-pixel tile (TR = 4 for
// 64 output channels, 2 for 128)
bool conv3s2w_eligible(const ConvShape& s);
int conv3s2w_tiles(const ConvLaunch& p);
int launch_conv3s2w(const ConvLaunch& p, hipStream_t st);
// nn.SpatialFullConvolution with stride 2..4 (`u<n>`, `f<k>s<s>-<n>`) by output phase on the physical input (kernels_tconv.hip); p = the
// PHYSICAL input with the module's own k / stride / pad; wpk = conv_tconv_pack() of the [cin][cout][k][k] weights (tconv_pack.h); partials
// per (8 x 32 input-pixel tile, phase) with explicit counts
bool conv_tconv_eligible(const ConvShape& s);
int conv_tconv_tiles(const ConvLaunch& p);
int launch_conv_tconv(const ConvLaunch& p, hipStream_t st);
// One enumerator per launch wrapper above.  fav_net picks one per layer (net.cpp: select_conv) and reports it through
// fav_net_profile_read_host as a kernel id -- a contract: bench.py, scripts/wide_bench.py and the GPU tests read the ids.  Everything else
// fav_net knows about a kernel -- its profile id among it -- is that kernel's row of CONV_KERNEL_TABLE (net_model.cpp)
enum ConvKernel { CK_GENERIC, CK_FOLD, CK_C8, CK_C8D, CK_FIRST1D, CK_FIRST2D, CK_S2W, CK_UP2, CK_WINO, CK_WINO4, CK_HALO3, CK_S2HALO, CK_TCONV };
constexpr int CONV_KERNELS = CK_TCONV + 1;      // (the last enumerator)
// kernels_elem.hip.  Per-channel finalize of (mean, M2) partials -> scale/shift:  scale = gamma/sqrt(var+eps)
// counts: per-partial pixel counts or null (then block b holds min(block_pixels, M - b*block_pixels) pixels)
int launch_in_finalize(const float* partials, const int* counts, int mblocks, int M, int block_pixels, int C, int Cpitch,
                       const float* gamma, const float* beta, float eps,
                       float* scale, float* shift, hipStream_t st);
// statistics of t(x) over an NHWC tensor [M][C] -> partials [ceil(M/128)][C] float2
int launch_stats(const float* x, int M, int C, const Affine& t, float* partials, hipStream_t st);
// a padding layer INSIDE the network (padding_type reflect / replicate): out[y][x][:] = in[map(y - pt)][map(x - pl)][:] of the (optionally
// x2 nearest-upsampled) NHWC tensor `in` with row pitch `in_pitch` pixels; mode 0 mirrors without repeating the edge, 1 repeats the edge
int launch_pad_nhwc(const float* in, int Hp, int Wp, int in_pitch, int C, int ups, float* out, int pl, int pr, int pt, int pb, int mode, hipStream_t st);
// z[oy][ox][c] = y[oy][ox][c]*scale[c]+shift[c] + t(skip[oy+s][ox+s][c]).  partials != null: also the per-row-segment
// (mean, M2, count) statistics of z ([res_add_stat_blocks(OH, OW)][C] float2 + counts) for an InstanceNorm that follows the join
int launch_res_add(const float* y, const float* scale, const float* shift,
                   const float* skip, int SH, int SW, int shave, const Affine& skip_t,
                   int C, float* z, float* partials, int* counts, hipStream_t st, int skip_pitch = 0, const Affine* branch_acc = nullptr);
// (branch_acc: the branch's InstanceNorm as accumulators -- Affine::acc1 -- instead of scale / shift; plain joins only)
inline int res_add_stat_blocks(int OH, int OW) { return OH * ((OW + 127) / 128); }
// NCHW [C][H][W] -> NHWC [H+2p][W+2p][Cp] with reflection padding p and zero channels >= C
int launch_nchw_to_nhwc_pad(const float* in, int C, int H, int W, int pad, int Cp, float* out, hipStream_t st);
// NHWC [M][C] with transform -> NCHW [C][M]
int launch_nhwc_to_nchw(const float* in, int M, int C, const Affine& t, float* out, hipStream_t st);

#ifdef __HIPCC__
// counter RNG standing in for the reference's unseeded torch.rand (core.lua:109); oracle: vr_oracle.fill_uniform
__device__ __forceinline__ float fill_uniform(unsigned seed, unsigned index, unsigned c, unsigned y, unsigned x)
{
    unsigned k = seed * 0x9E3779B1u + index * 0x85EBCA77u + c * 0xC2B2AE3Du + y * 0x27D4EB2Fu + x * 0x165667B1u;
    k ^= k >> 15; k *= 0x2C1B3C6Du;
    k ^= k >> 12; k *= 0x297A2D39u;
    k ^= k >> 15;
    return (float)(k >> 8) * (1.0f / 16777216.0f);
}
#endif

// frame-level kernels (kernels_frame.hip / kernels_consistency.hip)
constexpr int MIN_FILTER_RMAX = 15;      // largest -occlusions_min_filter window: the erosion kernels' LDS tiles are sized for it
int launch_warp(const float* img, const float* flow, float* out, int B, int C, int H, int W, int Ho, int Wo,
                int border, hipStream_t st);
int launch_min_filter_f32(const float* cert, float* out, int H, int W, int r, hipStream_t st);
int launch_assemble(const float* frame, const float* warped, const float* cert, float* in7, int H, int W,
                    hipStream_t st);
// certainty preparation for the fused path: u8 mask (optionally inverted / multiplied by the
// fix_occlusions term) -> min-filtered float certainty [H][W]
int launch_cert_prepare(const uint8_t* mask, const float* backward_flo, int invert, int fix_occ, int border,
                        int r, float* cert_tmp, float* cert, int H, int W, hipStream_t st);
// fused A2+A6+A7+reflection pad: writes the padded NHWC8 network input
int launch_prep_input(const uint8_t* frame_hwc, const float* prev_rgb, int Hs, int Ws, const float* backward_flo,
                      const float* cert, int border, int H, int W, int pad, float* in8, hipStream_t st,
                      int fill_random = 0, unsigned seed = 0, unsigned index = 0, int* q0_out = nullptr);
int launch_quantize_rgb8(const float* rgb_planar, uint8_t* out_hwc, int H, int W, hipStream_t st);
// long-term priors (kernels_longterm.hip): launch_prep_input with K = 1..FAV_LONG_TERM_MAX priors merged per pixel; the three arrays are
// HOST arrays of K device pointers (they travel in the kernel arguments); cert_out: the merged certainty [H][W] or null
int launch_longterm_prep(const uint8_t* frame_hwc, int K, const float* const* states, int Hs, int Ws, const float* const* backward_flo,
                         const float* const* cert, int border, int H, int W, int pad, float* in8, float* cert_out, hipStream_t st,
                         int fill_random = 0, unsigned seed = 0, unsigned index = 0);
// -scale_factor (kernels_scale.hip): image.scale(.., 'bicubic') [recalled].  launch_scale_prep: launch_prep_input for a frame without a
// prior, resampled H x W -> Hs x Ws on the way (in8: [Hs+2*pad][Ws+2*pad][8]; the fill is keyed by the scaled grid);
// launch_scale_planar: [C][Hs][Ws] -> [C][Hd][Wd] fp32
int launch_scale_prep(const uint8_t* frame_hwc, int H, int W, int Hs, int Ws, int pad, float* in8, hipStream_t st,
                      int fill_random = 0, unsigned seed = 0, unsigned index = 0);
int launch_scale_planar(const float* src, float* dst, int C, int Hs, int Ws, int Hd, int Wd, hipStream_t st);
// dense optical flow (kernels_flow.hip; tests/util/flow_model.py restates every stage).  Flows are .flo payloads [H][W][2]; `coef` is
// [H][W][4] (a, b, c, r), 16-byte aligned; launch_flow_sweeps runs `iters` Jacobi sweeps, up to K per launch, between *cur and *other
// and leaves the result in *cur.  Every launch works on `items` equal-sized planes at once (grid z): item j of an argument is p[j] of its
// FlowPtrs, a table that goes into the kernel arguments by value (2 x FAV_FLOW_MAX_PAIRS flows or images at most)
constexpr int FLOW_MAX_SWEEPS_PER_LAUNCH = 16;
constexpr int FLOW_MAX_ITEMS = 2 * FAV_FLOW_MAX_PAIRS;
struct FlowPtrs {
    void* p[FLOW_MAX_ITEMS];
    FlowPtrs() : p{} {}
    explicit FlowPtrs(const void* one) : p{} { p[0] = const_cast<void*>(one); }
    FlowPtrs(void* base, size_t stride_bytes, int items) : p{} { for (int j = 0; j < items; ++j) p[j] = static_cast<char*>(base) + j * stride_bytes; }
};
int launch_flow_grey(const FlowPtrs& rgb_hwc, const FlowPtrs& grey, int items, int W, int H, hipStream_t st);
int launch_flow_down(const FlowPtrs& src, int W, int H, const FlowPtrs& dst, int items, hipStream_t st);   // dst: ceil(W/2) x ceil(H/2)
int launch_flow_up(const FlowPtrs& coarse, int Wc, int Hc, const FlowPtrs& fine, int items, int W, int H, hipStream_t st);
// The variant of the coefficient and sweep launches.  wgt: the edge weights of the edge-preserving smoothness (smooth_eps > 0), [H][W][4]
// (n_l, n_r, n_u, n_d), 16-byte aligned -- written by launch_flow_coef from flow0 and `eps`, read by the sweeps; nullptr: the quadratic
// term (eps is not read).  grad: the gradient-constancy data term (tests/util/flow_grad_model.py); `coef` is then five planes [5][H][W]
// (q11, q12, q22, e1, e2), 4-byte aligned
// prior: the matching prior (tests/util/flow_match_model.py), nullptr = off: per flow three planes [3][ph][pw] = (d.x, d.y, m) of the level
// (shift 0, sx = sy = 1) or of level 1 when the launch is level 0's (shift 1: the parent sample, d times (sx, sy)); `coef` is then the
// five planes with either data term, and the sweeps are the gradient term's
constexpr int FLOW_MATCH_MAX_RADIUS = 32;
struct FlowPrior { FlowPtrs planes; int pw, ph, shift; float sx, sy, beta, tau; };
struct FlowVariant { float alpha; float eps; bool grad; const FlowPtrs* wgt; const FlowPrior* prior = nullptr; };
int launch_flow_coef(const FlowPtrs& A, const FlowPtrs& B, const FlowPtrs& flow0, const FlowPtrs& coef, const FlowVariant& v, int items, int W, int H,
                     hipStream_t st);
int launch_flow_sweeps(FlowPtrs* cur, FlowPtrs* other, const FlowPtrs& coef, const FlowVariant& v, int items, int iters, int K, int W, int H, hipStream_t st);
// the matching prior's stages: d [H][W] of short2 (dx, dy) per item from two grey planes; the forward-backward test of two such fields into
// the prior planes (d.x, d.y, m) of the first; the planes of the next coarser level, ceil(W/2) x ceil(H/2)
int launch_flow_match(const FlowPtrs& A, const FlowPtrs& B, const FlowPtrs& d, int items, int W, int H, int radius, hipStream_t st);
int launch_flow_match_check(const FlowPtrs& d_ab, const FlowPtrs& d_ba, const FlowPtrs& prior, int items, int W, int H, hipStream_t st);
int launch_flow_prior_down(const FlowPtrs& src, int W, int H, const FlowPtrs& dst, int items, hipStream_t st);
// the options of an entry from before data_term existed: its fav_flow_opts (or none) with the brightness term
inline fav_flow_opts_ex flow_opts_brightness(const fav_flow_opts* o) { return {o ? *o : fav_flow_opts{0, 0, 0, 0.f, 0, 0.f}, FAV_FLOW_DATA_BRIGHTNESS}; }
// ... and of one from before the matching prior existed: its fav_flow_opts_ex (or none) with the prior off
inline fav_flow_opts_ex2 flow_opts_no_match(const fav_flow_opts_ex* o) { return {o ? *o : flow_opts_brightness(nullptr), 0.f, 0}; }
// the median filter between warps (tests/util/flow_median_model.py): u and v of every item, each replaced by the median of its
// size x size window (size 3 | 5, indices clamped to the image), from src into dst; src and dst are distinct buffers
int launch_flow_median(const FlowPtrs& src, const FlowPtrs& dst, int items, int W, int H, int size, hipStream_t st);
// ... and the options of an entry from before the median filter existed: its fav_flow_opts_ex2 (or none) with the filter off
inline fav_flow_opts_ex3 flow_opts_no_median(const fav_flow_opts_ex2* o) { return {o ? *o : flow_opts_no_match(nullptr), 0}; }
// Huffman codes of the PNG encoder (png_tables.cpp): PNG_NTABLES model codes with their dynamic-block headers + the fixed code
constexpr int PNG_NSYM = 277;            // literals 0..255, end of block 256, length symbols 257..276 (runs of 3..66)
constexpr int PNG_NTABLES = 12;
constexpr int PNG_HDR_WORDS = 40;
struct PngTable {
    uint32_t sym[PNG_NSYM];              // (code length << 16) | bit-reversed code
    uint32_t hdr[PNG_HDR_WORDS];         // the block header behind BFINAL / BTYPE, LSB first
    uint32_t hdr_bits, btype, dist_len, dist_code;
};
const std::vector<PngTable>& png_tables();
size_t png_capacity(int W, int H);
size_t png_workspace_bytes(int W, int H);
uint32_t png_crc32_combine_host(uint32_t crc_a, uint32_t crc_b, uint32_t len_b);
int launch_png_encode(const uint8_t* rgb_hwc, const float* rgb_planar, int W, int H, void* png_out, size_t capacity, uint32_t* png_bytes,
                      void* workspace, size_t ws_bytes, hipStream_t st);
// 8-bit YCbCr planes <-> RGB (kernels_yuv.hip); the format has been validated (yuv_format_check, api.cpp).  launch_rgb_to_yuv takes
// exactly one of rgb_hwc / rgb_planar.
size_t yuv_frame_bytes(int W, int H, const fav_yuv_format& f);
int yuv_format_check(const char* who, int W, int H, const fav_yuv_format* f);
int launch_yuv_to_rgb8(const uint8_t* yuv, int W, int H, const fav_yuv_format& f, uint8_t* rgb_hwc, hipStream_t st);
int launch_rgb_to_yuv(const uint8_t* rgb_hwc, const float* rgb_planar, int W, int H, const fav_yuv_format& f, uint8_t* yuv, hipStream_t st);
// the same for every layout of include/fav_yuv.h (kernels_yuv_layout.hip: 4:2:2, 9 .. 16 bits; depth 8 in 4:2:0 / 4:4:4 goes to the
// launchers above); the layout has been validated (yuv_layout_check, api.cpp)
size_t yuv_layout_frame_bytes(int W, int H, const fav_yuv_layout& l);
int yuv_layout_check(const char* who, int W, int H, const fav_yuv_layout* l);
int launch_yuv_layout_to_rgb8(const void* yuv, int W, int H, const fav_yuv_layout& l, uint8_t* rgb_hwc, hipStream_t st);
int launch_rgb_to_yuv_layout(const uint8_t* rgb_hwc, const float* rgb_planar, int W, int H, const fav_yuv_layout& l, void* yuv, hipStream_t st);
// the stylised frame's luminance on the original frame's colours (kernels_color.hip; tests/util/color_model.py), as an RGB8 image or as
// the planes of that image; sizes, matrix and format have been validated (api.cpp)
int launch_color_transfer_rgb8(const float* state, const uint8_t* orig_hwc, int W, int H, int matrix, uint8_t* out_hwc, hipStream_t st);
int launch_color_transfer_yuv(const float* state, const uint8_t* orig_hwc, int W, int H, const fav_yuv_format& f, uint8_t* yuv, hipStream_t st);
// the block-histogram distance of two RGB8 frames (kernels_scene.hip; tests/util/scene_model.py): the workspace is zeroed by the call,
// the 17 integers go to `result` (device or host-mapped memory); W, H >= 4 and W * H <= 2^28 have been checked (api.cpp)
size_t scene_change_workspace_bytes();
int launch_scene_change(const uint8_t* prev_rgb_hwc, const uint8_t* cur_rgb_hwc, int W, int H, void* workspace, fav_scene_change* result, hipStream_t st);
int launch_check_cert(const float* backward_flo, const float* forward_flo, const float* structure, const float* avg, uint8_t* mask_out,
                      int invert, int fix_occ, int border, int r, float* cert, int H, int W, hipStream_t st);
// ... and the input assembly on top of it (launch_check_cert + launch_prep_input in one launch; round 5)
int launch_check_prep(const uint8_t* frame_hwc, const float* prev_rgb, int Hs, int Ws, const float* backward_flo, const float* forward_flo,
                      const float* structure, const float* avg, uint8_t* mask_out, float* cert, int invert, int fix_occ, int border, int r,
                      int H, int W, int pad, float* in8, hipStream_t st, int fill_random, unsigned seed, unsigned index);
int launch_store_flag(uint32_t* flag_host, uint32_t value, hipStream_t st);
int launch_unpad_input(const float* in8, int H, int W, int pad, float* in7, hipStream_t st);
int launch_temporal_loss(const float* prev_rgb, const float* cur_rgb, const float* backward_flo, const uint8_t* cert_u8, int border,
                         int H, int W, double* partial256, hipStream_t st);

size_t structure_workspace_bytes(int W, int H);
int launch_structure(const uint8_t* rgb_hwc, int W, int H, void* ws, size_t ws_bytes,
                     const float** structure_out, const float** avg_out, hipStream_t st, int pack_cus = 0, const int* q0_main = nullptr,
                     int* form_ran = nullptr);
int launch_structure_map(const uint8_t* rgb_hwc, int W, int H, void* ws, size_t ws_bytes, float* structure_out, float* avg_out,
                         int pack_cus, int q0, int* form_ran, hipStream_t st);
int launch_sequential_sum(const float* x, size_t n, float* sum_out, hipStream_t st);
int launch_consistency(const float* f1_flo, const float* f2_flo, const float* structure, const float* avg,
                       uint8_t* out, int W, int H, hipStream_t st);

// cube-map orchestration kernels (kernels_vr.hip)
int launch_vr_rotate(const float* src, float* dst, int H, int W, int mode, hipStream_t st);           // 1: +90, 2: -90, 3: 180
int launch_vr_accum(float* acc, const float* w, const float* div, size_t n, int first, hipStream_t st);
int launch_vr_cert(const uint8_t* cert_u8, const float* m0, const float* m1, const float* m2, const float* m3, float* out, size_t n,
                   hipStream_t st);
// launch_consistency + launch_vr_cert in one pass: mask_out[i] = consistency_pixel(bw, fw, structure, avg), out = max(mask / 255, m0..m3)
int launch_vr_check_cert(const float* bw_flo, const float* fw_flo, const float* structure, const float* avg, const float* m0,
                         const float* m1, const float* m2, const float* m3, uint8_t* mask_out, float* out, int H, int W, hipStream_t st);
int launch_vr_prior(const float* lfw, const float* border, const float* grad, const float* cert, const float* m, const float* m2,
                    float* out, size_t n, hipStream_t st);
int launch_vr_blend(const float* seg, const float* borders, const float* g, const float* anti, float* out, size_t n, hipStream_t st);
int launch_vr_median(const float* src, float* dst, int H, int W, int r, hipStream_t st);
int launch_vr_strip(const float* face, int FH, int FW, int cy, int cx, int CH, int CW, int mode, float* strip, int SH, int SW,
                    int x0, hipStream_t st);
int launch_vr_prep(const uint8_t* frame_hwc, const float* prior, const float* cert, int fill_random, unsigned seed, unsigned index,
                   int H, int W, int pad, float* in8, hipStream_t st);
// one equirectangular frame -> the six expanded cube faces (kernels_equi.hip); faces_u8 / faces_f32_or_null: HOST arrays of 6 device pointers
int launch_equi_to_faces(const uint8_t* equi_rgb_hwc, int ew, int eh, int hplus, int wplus, int overlap_w, int overlap_h, int supersample,
                         uint8_t* const* faces_u8, float* const* faces_f32_or_null, hipStream_t st);
int launch_vr_flo_to_lua(const float* flo_uv, float* lua_dydx, size_t n, hipStream_t st);

}  // namespace fav

struct fav_net;
namespace fav {
int net_device(const fav_net* n);
int net_pad(const fav_net* n);
int net_in_channels(const fav_net* n);
void net_out_size(const fav_net* n, int H, int W, int* Ho, int* Wo);
int net_forward_padded(fav_net* n, const float* in8, int H, int W, float* out_planar, hipStream_t st);
void net_forget_stream(const fav_net* n, hipStream_t st);      // `st` is about to be destroyed: drain it, never synchronise it again
void net_reserve_cus(fav_net* n, int cus);                      // the persistent / stream-K grids leave at least `cus` CUs to side queues
}  // namespace fav

