// net.cpp -- host side of the transformer network (A8): the device form of the weights, kernel selection, the executor, fav_net's C ABI.
//
// fav_net  : replaces `checkpoint.model` + `model:forward(input)` (fast_artistic_video_core.lua:38-57,172).
//
// Execution model ("lazy activations"): every activation lives in HBM exactly once, as the RAW output
// of the kernel that produced it (NHWC fp32).  nn.InstanceNormalization / nn.ReLU /
// nn.SpatialUpSamplingNearest never run as kernels of their own: they become a pending per-channel
// transform + index map attached to the tensor and are applied by the NEXT convolution while it
// stages its operand into LDS.  The InstanceNorm statistics come from the producing convolution's
// epilogue (per-tile mean/M2, merged in fp64), or -- when the normalised tensor is itself a pending
// transform of another tensor (the IN that follows an upsample of an already normalised+rectified
// tensor, models_video.lua:94-98,121-130) -- from one read-only reduction pass.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>

#include <mutex>

#include "fav_internal.h"
#include "wino_pack.h"
#include "wino4_pack.h"
#include "up2_pack.h"
#include "s2_pack.h"
#include "tconv_pack.h"
#include "first_pack.h"
#include "first2d_pack.h"
#include "fold_pack.h"

using namespace fav;

namespace {

struct DevBuf { void* p = nullptr; size_t bytes = 0; };
struct DevConvW {
    float* wgt = nullptr; float* bias = nullptr; unsigned short* wgt16 = nullptr;      // repack_weights() form: the generic, c8 and halo-resident kernels
    float* packed[CONV_KERNELS] = {};      // by ConvKernel: the form that kernel's own packing gives (upload_layers); null: that kernel cannot be selected
    int cinp = 0, coutp = 0, kpad = 0;
};
struct DevIN { float* gamma = nullptr; float* beta = nullptr; float* scale = nullptr; float* shift = nullptr;
               long long* acc = nullptr; size_t acc_bytes = 0; };      // accumulator form of the statistics (fav_internal.h, Affine::acc1): [2 parities][stat_acc_words(C)], zero between frames

struct Act {
    float* data = nullptr;
    int Hp = 0, Wp = 0;          // physical size
    int C = 0;                   // channel pitch
    int ups = 0;                 // pending nearest upsample (log2)
    Affine pre;                  // pending per-channel transform
    float* partials = nullptr;   // (mean, M2) tiles of the raw tensor from the producing conv, or null
    int mblocks = 0, ppitch = 0;
    int* counts = nullptr;       // per-partial pixel counts (first-layer kernel) or null
    int pitch = 0;               // row pitch in pixels when the tensor sits inside a wider allocation (0: Wp)
    // pending residual join (conv3_wino_kernel MODE 2): data = the branch's raw output, pre = its InstanceNorm, join_skip = the skip
    // tensor's pixel under data's pixel (0, 0) at the same pitch; join_out = where the consuming convolution writes the joined tensor
    const float* join_skip = nullptr; float* join_out = nullptr;
    long long* acc = nullptr; long long* acc_other = nullptr;      // the producing convolution added its statistics to accumulators (this frame's parity | the other one)
    int H() const { return Hp << ups; }
    int W() const { return Wp << ups; }
    int P() const { return pitch ? pitch : Wp; }
};

int dev_upload(const std::vector<float>& h, size_t pad_to, float** out)
{
    const size_t n = std::max(pad_to, h.size());
    std::vector<float> tmp(n, 0.f);
    std::copy(h.begin(), h.end(), tmp.begin());
    FAV_HIP(hipMalloc(reinterpret_cast<void**>(out), (n ? n : 1) * sizeof(float)));
    if (n) FAV_HIP(hipMemcpy(*out, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice));
    return FAV_OK;
}

// repack [cout][cin][k][k] -> [coutp][kpad].  K order of the implicit GEMM (must match FAV_TAP_SETUP):
//   cinp >= 32: k = ((ci/32)*taps + tap)*32 + ci%32   (channel slice outermost: consecutive K-steps shift by one tap)
//   cinp <  32: k = tap*cinp + ci                     (several taps per 32-wide K slice)
// nn.SpatialFullConvolution (weight [cin][cout][k][k]) runs as a stride-1 convolution over the zero-stuffed input with the
// taps flipped: out[oy] = sum_ky' stuffed[oy + ky' - (k-1-p)] * w[k-1-ky'].
void repack_weights(const Layer& L, int cinp, int coutp, int kpad, std::vector<float>& out)
{
    out.assign((size_t)coutp * kpad, 0.f);
    const int taps = L.k * L.k;
    for (int co = 0; co < L.cout; ++co)
        for (int ci = 0; ci < L.cin; ++ci)
            for (int ky = 0; ky < L.k; ++ky)
                for (int kx = 0; kx < L.k; ++kx) {
                    const int tap = ky * L.k + kx;
                    const size_t k = cinp >= 32 ? ((size_t)(ci / 32) * taps + tap) * 32 + ci % 32 : (size_t)tap * cinp + ci;
                    out[(size_t)co * kpad + k] = L.transposed
                        ? L.w[(((size_t)ci * L.cout + co) * L.k + (L.k - 1 - ky)) * L.k + (L.k - 1 - kx)]
                        : L.w[(((size_t)co * L.cin + ci) * L.k + ky) * L.k + kx];
                }
}

// Tuning / ablation switches (not part of the product contract): read ONCE per process, never on the launch path.
struct Tuning {
    // FAV_NO_<kernel>: select_conv() passes that kernel over
    bool no_fold = diag_env("FAV_NO_FOLD") != nullptr;
    bool no_c8 = diag_env("FAV_NO_C8") != nullptr;
    bool no_c8d = diag_env("FAV_NO_C8D") != nullptr;
    bool no_first = diag_env("FAV_NO_FIRST") != nullptr;
    bool no_s2w = diag_env("FAV_NO_S2W") != nullptr;
    bool no_up2 = diag_env("FAV_NO_UP2") != nullptr;
    bool no_wino = diag_env("FAV_NO_WINO") != nullptr;
    bool no_h3 = diag_env("FAV_NO_H3") != nullptr;
    bool no_s2 = diag_env("FAV_NO_S2") != nullptr;
    bool no_tconv = diag_env("FAV_NO_TCONV") != nullptr;              // transposed convolutions on the generic kernel, over the zero-stuffed input (stride 2, adj 1 only)
    bool first_1d = diag_env("FAV_FIRST_1D") != nullptr;              // the 1-D form of the first layer
    bool wino_f2 = diag_env("FAV_WINO_F2") != nullptr;                // the residual convolutions as F(2x2,3x3) (rounds 2-3) instead of F(4x4,3x3)
    bool no_acc_stats = diag_env("FAV_NO_ACC_STATS") != nullptr;      // every InstanceNorm through partials + an in_finalize launch (rounds 1-4)
    bool no_lazy_join = diag_env("FAV_NO_LAZY_JOIN") != nullptr;      // no residual join stays pending | with the F(4x4) kernels too (run(), L_RES)
    bool lazy_join = diag_env("FAV_LAZY_JOIN") != nullptr;
    int side_sk = diag_env("FAV_SIDE_SK") ? atoi(diag_env("FAV_SIDE_SK")) : 0;      // 1: stream-K stays next to the side queues, 2: for the stride-2 halo kernel only
};
const Tuning& tuning() { static const Tuning t; return t; }

// Which kernel runs convolution L (weights d) on an input with `stages` pending normalisations and a pending x`2^ups` upsampling -- the
// whole priority list, first match wins.  A kernel whose weights are not packed (d.packed[k] null: upload_layers) is never chosen.
// is_final: the network's last layer (Tanh epilogue) on an IH x IW logical input.  Also asked about LATER layers (acc_stats_ok,
// res_block_is_winograd), so it depends on nothing but its arguments.
ConvKernel select_conv(const Layer& L, const DevConvW& d, int stages, int ups, int precision, bool is_final, int IH, int IW, const Tuning& t)
{
    // only the generic kernel and the row-folded one (few output channels: kx taps folded into N) have the Tanh epilogue
    if (is_final) return !t.no_fold && d.packed[CK_FOLD] && conv_fold_launchable(d.cinp, L.k, L.pad, ups, IH, IW) ? CK_FOLD : CK_GENERIC;
    // a transposed convolution (stride >= 2: upload() turns stride 1 into an ordinary convolution) by output phase on the physical input;
    // FAV_NO_TCONV: on the generic kernel, over the zero-stuffed input
    if (L.transposed) return !t.no_tconv && d.packed[CK_TCONV] && conv_tconv_eligible(d.cinp, d.coutp, L.k, L.stride, L.pad, L.adj, ups) ? CK_TCONV : CK_GENERIC;
    // The first layer (9x9 on the 8-channel input pixel) by minimal filtering, ahead of its direct forms below: 2-D F(2x2,3x3) over its
    // nine 3x3 blocks, or 1-D F(2,3) along x on request (FAV_FIRST_1D).  FAV_NO_C8D takes both away together with the dense-K direct
    // form.  A layer that the c8 kernel does not take (more than 32 filters, FAV_NO_C8) has the 2-D form only, in groups of 32 filters
    const bool c8 = !t.no_c8 && conv_c8_eligible(d.cinp, d.coutp, L.k, L.stride, stages, ups);
    if (!t.no_first && !t.no_c8d) {
        if (c8 && d.packed[CK_FIRST1D] && conv_c8d_eligible(d.cinp, L.cin, d.coutp, L.k, L.stride, stages, ups))
            return d.packed[CK_FIRST2D] && !t.first_1d ? CK_FIRST2D : CK_FIRST1D;
        if (!c8 && d.packed[CK_FIRST2D] && conv_first2d_eligible(d.cinp, L.cin, d.coutp, L.k, L.stride, stages, ups)) return CK_FIRST2D;
    }
    // 3x3 stride 2 (d64 / d128): the fragment-order kernel, ahead of the stride-2 halo kernel and the generic one that ran them before it
    if (d.packed[CK_S2W] && !t.no_s2w && conv3s2w_eligible(d.cinp, L.cout, d.coutp, L.k, L.stride, L.pad, stages, ups)) return CK_S2W;
    // 3x3 on a x2-upsampled input (fp32 only): four 2x2 convolutions on the physical pixels instead of a 3x3 on every logical one
    if (d.packed[CK_UP2] && precision == 0 && !t.no_up2 &&
        conv3_up2_eligible(d.cinp, L.cout, d.coutp, L.k, L.stride, L.pad, stages, ups)) return CK_UP2;
    // unpadded 3x3 stride 1 (the residual blocks; fp32 only): Winograd F(4x4) where it is packed (not under FAV_WINO_F2), else F(2x2)
    if (precision == 0 && !t.no_wino) {
        if (d.packed[CK_WINO4] && conv3_wino4_eligible(d.cinp, L.cout, d.coutp, L.k, L.stride, L.pad, stages, ups)) return CK_WINO4;
        if (d.packed[CK_WINO] && conv3_wino_eligible(d.cinp, L.cout, d.coutp, L.k, L.stride, L.pad, stages, ups)) return CK_WINO;
    }
    // the first layer's direct forms: dense K for its 7 (3) real input channels, else all 8
    if (c8) return !t.no_c8d && d.packed[CK_C8D] && conv_c8d_eligible(d.cinp, L.cin, d.coutp, L.k, L.stride, stages, ups) ? CK_C8D : CK_C8;
    // the halo-resident implicit GEMMs take what is left of the 3x3 layers (bf16 fast mode, padded layers, FAV_NO_WINO / _UP2 / _S2W)
    if (!t.no_h3 && conv3_halo_eligible(d.cinp, d.coutp, L.k, L.stride)) return CK_HALO3;
    if (!t.no_s2 && conv3s2_eligible(d.cinp, d.coutp, L.k, L.stride, stages, ups)) return CK_S2HALO;
    return CK_GENERIC;
}

// What run() and timed_conv() need to know about each kernel: how many partial-statistics tiles it writes for an OH x OW output, whether
// it writes their pixel counts (else every tile but the last holds CONV_BM pixels), and its profile id (fav_internal.h, ConvKernel)
struct ConvFacts { int tiles; bool counts; int id; };
ConvFacts conv_facts(ConvKernel k, int OH, int OW, int coutp, int precision, bool join, int stride)
{
    switch (k) {
    case CK_GENERIC: return {conv_mblocks(OH, OW), false, coutp % 128 == 0 ? 128 : (coutp % 64 == 0 ? 64 : 32)};
    case CK_FOLD:    return {0, false, 1};      // (the last layer: nothing normalises its output)
    case CK_C8:      return {conv_c8_tiles(OH, OW), true, 8};
    case CK_C8D:     return {conv_c8_tiles(OH, OW), true, 7};
    case CK_FIRST1D: return {conv_first_tiles(OH, OW), true, 6};
    case CK_FIRST2D: return {conv_first2d_tiles(OH, OW), true, 16};
    case CK_S2W:     return {conv3s2w_tiles(OH, OW, coutp), true, 700 + coutp};
    case CK_UP2:     return {conv3_up2_tiles(OH, OW), true, 500 + coutp};
    case CK_WINO:    return {conv3_wino_tiles(OH, OW), true, 400 + coutp + (join ? 1 : 0)};
    case CK_WINO4:   return {conv3_wino4_tiles(OH, OW), true, 600 + coutp + (join ? 1 : 0)};
    case CK_HALO3:   return {conv3_halo_tiles(OH, OW, precision == 0), true, 300 + coutp};
    case CK_S2HALO:  return {conv3s2_tiles(OH, OW), true, 200 + coutp};
    case CK_TCONV:   return {conv_tconv_tiles(OH, OW, stride), true, 800 + coutp};
    }
    return {0, false, 0};
}

// The launch of kernel k with its packed weights.  cs: the full descriptor; cg: the same with no_sk set while look-ahead masks are in
// flight (timed_conv) -- for the kernels whose blocks hand tiles over to each other
int launch_selected(ConvKernel k, const ConvLaunch& cs, const ConvLaunch& cg, const DevConvW& d, int cin_real, int* counts, hipStream_t st)
{
    const float* w = d.packed[k];
    switch (k) {
    case CK_GENERIC: return launch_conv(cg, st);
    case CK_FOLD:    return launch_conv_fold(cs, w, st);
    case CK_C8:      return launch_conv_c8(cs, counts, st);
    case CK_C8D:     return launch_conv_c8d(cs, cin_real, w, counts, st);
    case CK_FIRST1D: return launch_conv_first(cs, cin_real, w, counts, st);
    case CK_FIRST2D: return launch_conv_first2d(cs, cin_real, w, counts, st);
    case CK_S2W:     return launch_conv3s2w(cs, w, counts, st);
    case CK_UP2:     return launch_conv3_up2(cs, w, counts, st);
    case CK_WINO:    return launch_conv3_wino(cs, w, counts, st);
    case CK_WINO4:   return launch_conv3_wino4(cs, w, counts, st);
    case CK_HALO3:   return launch_conv3_halo(cg, counts, st);
    case CK_S2HALO:  return launch_conv3s2(tuning().side_sk == 2 ? cs : cg, counts, st);
    case CK_TCONV:   return launch_conv_tconv(cs, w, counts, st);
    }
    set_error("internal: unknown convolution kernel %d", (int)k); return FAV_EINVAL;
}

// The input state a kernel is built for, as the (stages, ups) of its eligibility predicate: pack_weights() asks with it whether the
// kernel can EVER run the layer; select_conv() asks again per forward, with the state the input is then in
struct InputState { int stages, ups; };
constexpr InputState IN_PLAIN{0, 0};        // nothing pending: the network input (first layer); also asked for the residual 3x3 convolutions, which take 0 or 1 norms
constexpr InputState IN_NORM{1, 0};         // one pending norm (+ ReLU), no upsampling: the stride-2 layers
constexpr InputState IN_NORM_UP2{1, 1};     // one pending norm behind a x2 upsampling: up2

// true: `out` is kernel k's packed form of layer L; false: k cannot run L (or runs on the repack_weights() form) and d.packed[k] stays null
bool pack_weights(ConvKernel k, const Layer& L, const DevConvW& d, std::vector<float>& out)
{
    const float* w = L.w.data();
    if (L.transposed) {                  // [cin][cout][k][k]: the phase kernel's form, or (FAV_NO_TCONV) the generic kernel's flipped repack_weights() form
        if (k != CK_TCONV || !conv_tconv_eligible(d.cinp, d.coutp, L.k, L.stride, L.pad, L.adj, IN_PLAIN.ups)) return false;
        conv_tconv_pack(w, L.cin, L.cout, d.cinp, d.coutp, L.k, L.stride, L.pad, out); return true;
    }
    const bool first = conv_c8d_eligible(d.cinp, L.cin, d.coutp, L.k, L.stride, IN_PLAIN.stages, IN_PLAIN.ups);      // the first layer with at most 32 filters
    const bool full_k = L.cin == d.cinp;      // every channel of the input pitch is a real one (not the 7 | 3 network inputs in their 8-channel pixel)
    switch (k) {
    case CK_GENERIC: case CK_C8: case CK_HALO3: case CK_S2HALO:
        return false;      // d.wgt / d.wgt16
    case CK_C8D:           // first layer: dense-K pairing
        if (!first) return false;
        conv_c8d_pack(w, L.cin, L.cout, out); return true;
    case CK_FIRST1D:       // the same layer with F(2,3) along x (kernels_first.hip)
        if (!first) return false;
        conv_first_pack(w, L.cin, L.cout, out); return true;
    case CK_FIRST2D:       // ... and with F(2x2,3x3) over its nine 3x3 blocks; a first layer with more than 32 filters: groups of 32
        if (first) { conv_first2d_pack(w, L.cin, L.cout, out); return true; }
        if (!conv_first2d_eligible(d.cinp, L.cin, d.coutp, L.k, L.stride, IN_PLAIN.stages, IN_PLAIN.ups)) return false;
        conv_first2d_pack_groups(w, L.cin, L.cout, d.coutp, out); return true;
    case CK_WINO:          // residual 3x3: Winograd
        if (!full_k || !conv3_wino_eligible(d.cinp, L.cout, d.coutp, L.k, L.stride, L.pad, IN_PLAIN.stages, IN_PLAIN.ups)) return false;
        conv_wino_pack(w, L.cin, L.cout, out); return true;
    case CK_WINO4:         // ... as F(4x4,3x3) (round 4), any number of 128-filter groups (round 5)
        if (!full_k || tuning().wino_f2 || !conv3_wino4_eligible(d.cinp, L.cout, d.coutp, L.k, L.stride, L.pad, IN_PLAIN.stages, IN_PLAIN.ups)) return false;
        conv_wino4_pack_groups(w, L.cin, L.cout, out); return true;
    case CK_UP2:           // 3x3 after a x2 upsampling: merged 2x2 taps
        if (!full_k || !conv3_up2_eligible(d.cinp, L.cout, d.coutp, L.k, L.stride, L.pad, IN_NORM_UP2.stages, IN_NORM_UP2.ups)) return false;
        if (L.cout == 64) {
            std::vector<float> w9;
            conv_up2_pack(w, L.cin, out);
            conv_up2w_pack(w, L.cin, w9);                        // the nine-position form follows the phase-merged one
            out.insert(out.end(), w9.begin(), w9.end());
        } else conv_up2w_pack_groups(w, L.cin, L.cout, out);      // more than 64 filters: the nine-position form only, one block per group of 64
        return true;
    case CK_S2W:           // 3x3 stride 2: fragment order
        if (!full_k || !conv3s2w_eligible(d.cinp, L.cout, d.coutp, L.k, L.stride, L.pad, IN_NORM.stages, IN_NORM.ups)) return false;
        conv_s2w_pack_groups(w, L.cin, L.cout, out); return true;
    case CK_FOLD:          // the row-folded last layer
        if (!conv_fold_eligible(d.cinp, L.cout, L.k, L.stride)) return false;
        conv_fold_pack(w, L.cin, d.cinp, L.cout, L.k, out); return true;
    case CK_TCONV:         // (transposed layers only: above)
        return false;
    }
    return false;
}

// one more pending per-channel stage t(x) = relu?(x*scale+shift) on a tensor that carries at most one
int append_stage(Affine& a, const float* scale, const float* shift, int relu)
{
    if (a.stages >= 2) { set_error("network: more than two stacked normalisations on one tensor are unsupported"); return FAV_EUNSUPPORTED; }
    if (a.stages == 0) { a.scale1 = scale; a.shift1 = shift; a.relu1 = relu; }
    else { a.scale2 = scale; a.shift2 = shift; a.relu2 = relu; }
    ++a.stages;
    return FAV_OK;
}

bool only_tail(const std::vector<Layer>& ls, size_t from, bool& has_tanh, float& mul);
int pow2_ceil(int c) { int p = 4; while (p < c) p <<= 1; return p; }

// Channel pitches of the kernels are powers of two (the generic kernel locates (tap, channel) with shifts, the elementwise kernels
// split 256 threads over the channels).  Architectures with other filter counts -- models_video.lua:55-140 builds any `c9s1-48,d96,...`,
// the VR checkpoints have "more filters" (README.md:141) -- are EXECUTED as the next power of two with zero filters: a padded output
// channel has zero weights and zero bias (identically 0), its InstanceNorm / BatchNorm gets scale 0 and shift 0 (stays 0 through ReLU,
// residual joins and upsampling), and the next convolution has zero weights for it -- every real channel sees exactly the sums it saw
// before (x + 0 * 0 = x).  `chan`: channels of the tensor flowing in (already padded).  The 3-channel last layer keeps its size.
// `real`: the channel count the checkpoint itself gives that tensor (what a following InstanceNorm / BatchNorm / conv must match:
// a malformed file -- IN(64) behind a real 128-channel conv -- is rejected, not run with its upper channels forced to zero);
// `seen_conv`: false until the network's first convolution, whose 7 (3) inputs ride in an 8-channel pixel.
int pad_channel_counts(std::vector<Layer>& ls, int& chan, int& real, bool& seen_conv, bool top)
{
    for (size_t li = 0; li < ls.size(); ++li) {
        Layer& L = ls[li];
        if (L.type == L_CONV) {
            const bool first_input = !seen_conv && L.cin <= 8;           // the 7 (3) network inputs ride in an 8-channel pixel
            seen_conv = true;
            const int cin_new = first_input ? L.cin : chan;
            bool has_tanh = false; float mul = 1.f;
            const bool is_final = top && L.cout == 3 && only_tail(ls, li + 1, has_tanh, mul) && has_tanh;
            const int cout_new = is_final ? L.cout : pow2_ceil(L.cout);
            if (!first_input && L.cin != real) { set_error("network: conv expects %d input channels, its producer has %d", L.cin, real); return FAV_EFORMAT; }
            const int cout_real = L.cout;
            if (cin_new != L.cin || cout_new != L.cout) {
                std::vector<float> w((size_t)cout_new * cin_new * L.k * L.k, 0.f);
                const size_t kk = (size_t)L.k * L.k;
                for (int co = 0; co < L.cout; ++co)
                    for (int ci = 0; ci < L.cin; ++ci) {
                        const float* src = L.transposed ? &L.w[((size_t)ci * L.cout + co) * kk] : &L.w[((size_t)co * L.cin + ci) * kk];
                        float* dst = L.transposed ? &w[((size_t)ci * cout_new + co) * kk] : &w[((size_t)co * cin_new + ci) * kk];
                        std::copy(src, src + kk, dst);
                    }
                L.w.swap(w);
                if (!L.b.empty()) L.b.resize((size_t)cout_new, 0.f);
                L.cin = cin_new; L.cout = cout_new;
            }
            chan = L.cout; real = cout_real;
        } else if (L.type == L_IN) {
            if ((int)L.gamma.size() != real) { set_error("network: InstanceNormalization(%zu) after %d channels", L.gamma.size(), real); return FAV_EFORMAT; }
            L.gamma.resize((size_t)chan, 0.f); L.beta.resize((size_t)chan, 0.f);
        } else if (L.type == L_BN) {
            if ((int)L.mean.size() != real) { set_error("network: SpatialBatchNormalization(%zu) after %d channels", L.mean.size(), real); return FAV_EFORMAT; }
            L.gamma.resize((size_t)chan, 0.f); L.beta.resize((size_t)chan, 0.f); L.mean.resize((size_t)chan, 0.f); L.var.resize((size_t)chan, 1.f);
        } else if (L.type == L_RES) {
            int c = chan, r = real;
            int rc = pad_channel_counts(L.block, c, r, seen_conv, false); if (rc) return rc;
            if (c != chan || r != real) { set_error("network: residual branch changes the channel count"); return FAV_EUNSUPPORTED; }
        }
    }
    return FAV_OK;
}

// A stride-1 nn.SpatialFullConvolution (`f<k>s1-<n>`) IS an ordinary convolution: weights flipped and transposed to [cout][cin], zero
// padding k - 1 - p.  Rewritten in the executed copy of the network, so that it gets the ordinary kernels, the Tanh epilogue and the
// upsampled-input handling; describe / output size keep the module as the file has it
int rewrite_stride1_transposed(std::vector<Layer>& ls)
{
    for (Layer& L : ls) {
        if (L.type == L_RES) { int rc = rewrite_stride1_transposed(L.block); if (rc) return rc; }
        if (L.type != L_CONV || !L.transposed || L.stride != 1) continue;
        if (L.k < 1 || L.pad < 0 || L.pad > L.k - 1 || L.adj != 0) {
            set_error("network: SpatialFullConvolution with stride 1 needs pad <= k - 1 and adj 0, got k=%d pad=%d adj=%d", L.k, L.pad, L.adj);
            return FAV_EUNSUPPORTED; }
        std::vector<float> w;
        conv_tconv_as_conv(L.w.data(), L.cin, L.cout, L.k, w);
        L.w.swap(w); L.pad = L.k - 1 - L.pad; L.transposed = 0;
    }
    return FAV_OK;
}

long long count_params(const std::vector<Layer>& ls)
{
    long long n = 0;
    for (const Layer& L : ls) {
        if (L.type == L_CONV) n += (long long)L.w.size() + (long long)L.b.size();
        else if (L.type == L_IN) n += 2 * (long long)L.gamma.size();
        else if (L.type == L_BN) n += 4 * (long long)L.mean.size();
        else if (L.type == L_RES) n += count_params(L.block);
    }
    return n;
}

bool only_tail(const std::vector<Layer>& ls, size_t from, bool& has_tanh, float& mul)
{
    has_tanh = false; mul = 1.f;
    for (size_t i = from; i < ls.size(); ++i) {
        if (ls[i].type == L_TANH) { if (has_tanh) return false; has_tanh = true; }
        else if (ls[i].type == L_MUL) { if (!has_tanh) return false; mul *= ls[i].mul; }
        else if (ls[i].type != L_IDENTITY) return false;
    }
    return true;
}

}  // namespace

struct fav_net {
    int device = 0;
    std::vector<Layer> layers;    // as parsed from the checkpoint (describe / output size / parameter count)
    std::vector<Layer> exec;      // what runs: the same network with channel counts padded to powers of two (pad_channel_counts)
    int pad = 0;                  // leading nn.SpatialReflectionPadding (train_video.lua:319-325)
    bool pad_folded = false;      // ... folded into the input assembly (layers[0] is then skipped by the executor)
    int in_channels = 0;
    long long params = 0;
    std::vector<DevConvW> convs;  // traversal order
    std::vector<DevIN> ins;
    float* ones = nullptr; float* zeros = nullptr;
    float* sk_ws = nullptr; unsigned* sk_flags = nullptr; unsigned sk_epoch = 0;   // stream-K hand-off state
    float* ks_ws = nullptr; int* ks_cnt = nullptr;                                    // meeting places of the F(4x4) Winograd kernel's stream-K launches
    // a residual block whose join stays pending (run(), L_RES): its last convolution lays its output out under the skip tensor
    struct LazyOut { bool active = false; int pitch = 0, rows = 0, shave = 0, conv_index = -1; } lazy;
    unsigned* sk_err_host = nullptr; unsigned* sk_err_dev = nullptr;               // host-mapped: a hand-off wait timed out
    bool shared_device = false;     // data-parallel grids only: set by the caller (fav_net_set_shared_device) or by a timed-out hand-off
    int precision = 0;              // 0 = fp32 (parity mode), 1 = bf16 operands in the halo-resident 3x3 convolutions (fast mode)
    int acc_parity = 0;             // which half of the InstanceNorm accumulators this forward adds to (the consumers zero the other half)
    bool acc_dirty = false;         // a forward failed half-way (or the precision changed): every accumulator is zeroed before the next forward
    bool branch_tail_acc_ok = false; // set by L_RES around its branch: the join is a plain res_add launch, which takes the last InstanceNorm as accumulators
    int reserve_cus = 0;            // set when a stream uses the look-ahead side queues (they are CU-masked to this many CUs)
    // activation arena: buffers are created on the first forward for a given (H, W) and reused after
    int curH = 0, curW = 0;
    std::vector<DevBuf> bufs;
    // ... carved out of a few large slabs: sixty hipMalloc calls cost the first frame of a run 10 ms (profiles/e2e_r04s_startup.log)
    std::vector<void*> slabs; char* slab_cur = nullptr; size_t slab_left = 0;
    size_t cursor = 0, conv_cursor = 0, in_cursor = 0;
    hipStream_t st = nullptr;
    float* stage = nullptr; size_t stage_bytes = 0;   // NCHW-boundary staging (fav_net_forward)
    // optional per-convolution event timing (bench.py roofline)
    bool profiling = false;
    struct ProfRec { hipEvent_t a, b; int conv; };
    std::vector<ProfRec> prof_pending;
    std::vector<double> prof_ms, prof_macs; std::vector<int> prof_n, prof_tile;

    ~fav_net()
    {
        (void)hipSetDevice(device);
        (void)hipFree(stage);
        for (auto& c : convs) { (void)hipFree(c.wgt); (void)hipFree(c.bias); (void)hipFree(c.wgt16); for (float* p : c.packed) (void)hipFree(p); }
        for (auto& i : ins) { (void)hipFree(i.gamma); (void)hipFree(i.beta); (void)hipFree(i.scale); (void)hipFree(i.shift); (void)hipFree(i.acc); }
        for (void* sp : slabs) (void)hipFree(sp);
        (void)hipFree(ones); (void)hipFree(zeros); (void)hipFree(sk_ws); (void)hipFree(sk_flags); (void)hipFree(ks_ws); (void)hipFree(ks_cnt); if (sk_err_host) (void)hipHostFree(sk_err_host);
    }
    int upload_layers(std::vector<Layer>& ls, int& chan_pitch, int& maxc);
    int upload();
    int alloc(size_t bytes, float** out);
    int timed_conv(const ConvLaunch& c, int conv_index, const Layer& L, ConvKernel kernel, int* counts);
    int run(std::vector<Layer>& ls, Act& cur, bool top, float* out_planar, float* out_raw);
    bool res_block_is_winograd(const Layer& R, size_t first_conv) const;
    bool acc_stats_ok(const std::vector<Layer>& ls, size_t li) const;
    int forward_padded(const float* in8, int H, int W, float* out_planar, float* out_raw, hipStream_t stream);
    int forward_padded_unordered(const float* in8, int H, int W, float* out_planar, float* out_raw, hipStream_t stream);
    void out_size(int H, int W, int* Ho, int* Wo) const;
};

int fav_net::upload_layers(std::vector<Layer>& ls, int& chan_pitch, int& maxc)
{
    for (Layer& L : ls) {
        if (L.type == L_CONV) {
            convs.emplace_back();                 // registered first: the destructor frees whatever a failed upload leaves behind
            DevConvW& d = convs.back();
            d.cinp = chan_pitch;
            if (L.cin > chan_pitch || (chan_pitch != 8 && L.cin != chan_pitch)) {
                set_error("network: conv expects %d input channels, producer has %d", L.cin, chan_pitch); return FAV_EFORMAT; }
            if (L.k < 1 || L.stride < 1 || L.pad < 0) { set_error("network: bad convolution geometry"); return FAV_EFORMAT; }
            // channel pitches are powers of two (the generic kernel locates (tap, channel) with shifts, the elementwise kernels split 256
            // threads over the channels): 4 ... 1024 -- every architecture string of models_video.lua / train_video.lua:21-23.  Refused
            // here, at load time: a 48-channel model used to overrun the repacked weight matrix before any launch could refuse it
            if ((d.cinp & (d.cinp - 1)) != 0) {
                set_error("network: a convolution with %d input channels is unsupported (channel counts must be powers of two)", d.cinp);
                return FAV_EUNSUPPORTED; }
            d.coutp = (L.cout + 31) / 32 * 32;
            d.kpad = (L.k * L.k * d.cinp + 31) / 32 * 32;
            // a transposed layer runs by output phase (CK_TCONV); the zero-stuffed form on the generic kernel -- a x2 index map: stride 2,
            // adj 1 ONLY -- is what is left for a layer the phase kernel does not take (a 4-channel input pitch), and for FAV_NO_TCONV
            const bool phase = L.transposed && !tuning().no_tconv && conv_tconv_eligible(d.cinp, d.coutp, L.k, L.stride, L.pad, L.adj, IN_PLAIN.ups);
            if (L.transposed && !phase && (L.stride != 2 || L.adj != 1) && L.stride >= 2 && L.stride <= TCONV_MAX_S && L.k <= TCONV_MAX_K && L.pad <= L.k - 1 && L.adj >= 0 && L.adj < L.stride) {
                if (tuning().no_tconv) set_error("network: the zero-stuffed form of SpatialFullConvolution (diagnostic switch) is stride 2, adj 1 only, got s=%d adj=%d", L.stride, L.adj);
                else set_error("network: SpatialFullConvolution with s=%d adj=%d behind %d input channels is unsupported (other than stride 2, adj 1 it needs a multiple of 8)", L.stride, L.adj, d.cinp);
                return FAV_EUNSUPPORTED; }
            std::vector<float> w;
            int rc = FAV_OK;
            if (!phase) {                   // (the phase kernel reads its own packing only: no generic weight matrix for it)
                repack_weights(L, d.cinp, d.coutp, d.kpad, w);
                rc = dev_upload(w, 0, &d.wgt); if (rc) return rc;
            }
            rc = dev_upload(L.b, (size_t)d.coutp, &d.bias); if (rc) return rc;
            if (!L.transposed && conv3_halo_eligible(d.cinp, d.coutp, L.k, L.stride)) {      // bf16 copy for the fast mode (round to nearest even)
                std::vector<unsigned short> w16(w.size());
                for (size_t i = 0; i < w.size(); ++i) { unsigned b; memcpy(&b, &w[i], 4); w16[i] = (unsigned short)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16); }
                FAV_HIP(hipMalloc(reinterpret_cast<void**>(&d.wgt16), w16.size() * 2));
                FAV_HIP(hipMemcpy(d.wgt16, w16.data(), w16.size() * 2, hipMemcpyHostToDevice));
            }
            if (L.transposed && (L.k > TCONV_MAX_K || L.stride < 2 || L.stride > TCONV_MAX_S || L.pad > L.k - 1 || L.adj < 0 || L.adj >= L.stride)) {
                set_error("network: SpatialFullConvolution is supported for k <= %d, stride <= %d, pad <= k - 1, adj < stride (models_video.lua:81-89,99-102), got k=%d s=%d pad=%d adj=%d",
                          TCONV_MAX_K, TCONV_MAX_S, L.k, L.stride, L.pad, L.adj);
                return FAV_EUNSUPPORTED; }
            std::vector<float> wk;      // every kernel's own form of the weights: null where pack_weights() has none
            for (int k = 0; k < CONV_KERNELS; ++k)
                if (pack_weights((ConvKernel)k, L, d, wk)) { rc = dev_upload(wk, 0, &d.packed[k]); if (rc) return rc; }
            chan_pitch = L.cout;
            maxc = std::max(maxc, std::max(d.coutp, d.cinp));
        } else if (L.type == L_IN) {
            if ((int)L.gamma.size() != chan_pitch) { set_error("network: InstanceNormalization(%zu) after %d channels", L.gamma.size(), chan_pitch); return FAV_EFORMAT; }
            ins.emplace_back();
            DevIN& d = ins.back();
            int rc = dev_upload(L.gamma, 0, &d.gamma); if (rc) return rc;
            rc = dev_upload(L.beta, 0, &d.beta); if (rc) return rc;
            FAV_HIP(hipMalloc(reinterpret_cast<void**>(&d.scale), L.gamma.size() * sizeof(float)));
            FAV_HIP(hipMalloc(reinterpret_cast<void**>(&d.shift), L.gamma.size() * sizeof(float)));
            d.acc_bytes = 2 * stat_acc_words((int)L.gamma.size()) * sizeof(long long);
            FAV_HIP(hipMalloc(reinterpret_cast<void**>(&d.acc), d.acc_bytes));
            FAV_HIP(hipMemset(d.acc, 0, d.acc_bytes));
        } else if (L.type == L_BN) {
            if ((int)L.mean.size() != chan_pitch) { set_error("network: SpatialBatchNormalization(%zu) after %d channels", L.mean.size(), chan_pitch); return FAV_EFORMAT; }
            // evaluate mode: a fixed per-channel affine, folded into the consumer's load like InstanceNorm's
            std::vector<float> sc(L.mean.size()), sh(L.mean.size());
            for (size_t i = 0; i < sc.size(); ++i) {
                const double s = (double)L.gamma[i] / std::sqrt((double)L.var[i] + (double)L.eps);
                sc[i] = (float)s; sh[i] = (float)((double)L.beta[i] - (double)L.mean[i] * s);
            }
            ins.emplace_back();
            DevIN& d = ins.back();
            int rc = dev_upload(sc, 0, &d.scale); if (rc) return rc;
            rc = dev_upload(sh, 0, &d.shift); if (rc) return rc;
        } else if (L.type == L_RES) {
            int cp = chan_pitch;
            int rc = upload_layers(L.block, cp, maxc); if (rc) return rc;
            if (cp != chan_pitch) { set_error("network: residual branch changes the channel count"); return FAV_EUNSUPPORTED; }
        }
    }
    return FAV_OK;
}

int fav_net::upload()
{
    FAV_HIP(hipSetDevice(device));
    if (layers.empty()) { set_error("network: empty model"); return FAV_EFORMAT; }
    // A LEADING symmetric reflection padding (padding_type reflect-start: train_video.lua:319-325; also the pad in front of the first
    // convolution with padding_type reflect, models_video.lua:70-72) is folded into the input assembly (prep_input / check_prep write the
    // reflected copies).  Every other padding layer -- replication, asymmetric, or further inside the network (models_video.lua:12-16,27-31:
    // padding_type reflect / replicate pads in front of EVERY convolution) -- runs as a gather launch (launch_pad_nhwc).
    pad = 0; pad_folded = false;
    if (layers[0].type == L_PAD) {
        const Layer& P = layers[0];
        if (P.pad_mode == 0 && P.pl == P.pr && P.pl == P.pt && P.pl == P.pb) { pad = P.pl; pad_folded = true; }
    }
    in_channels = 0;
    for (const Layer& L : layers) if (L.type == L_CONV) { in_channels = L.cin; break; }
    if (in_channels != 7 && in_channels != 3) {
        set_error("network: first convolution has %d input channels; video models take 7 (models_video.lua:57), image models 3", in_channels);
        return FAV_EUNSUPPORTED; }
    exec = layers;
    int rc = rewrite_stride1_transposed(exec); if (rc) return rc;
    int chan0 = 8;
    int real0 = in_channels; bool seen_conv = false;
    rc = pad_channel_counts(exec, chan0, real0, seen_conv, true); if (rc) return rc;
    int chan = 8, maxc = 8;
    rc = upload_layers(exec, chan, maxc); if (rc) return rc;
    params = count_params(layers);
    std::vector<float> o((size_t)maxc, 1.f), z((size_t)maxc, 0.f);
    rc = dev_upload(o, 0, &ones); if (rc) return rc;
    rc = dev_upload(z, 0, &zeros); if (rc) return rc;
    FAV_HIP(hipMalloc(reinterpret_cast<void**>(&sk_ws), conv_streamk_workspace_bytes()));
    FAV_HIP(hipMalloc(reinterpret_cast<void**>(&sk_flags), conv_streamk_grid() * sizeof(unsigned)));
    FAV_HIP(hipMemset(sk_flags, 0, conv_streamk_grid() * sizeof(unsigned)));
    FAV_HIP(hipMalloc(reinterpret_cast<void**>(&ks_ws), conv3_wino4_ksplit_bytes()));
    FAV_HIP(hipMalloc(reinterpret_cast<void**>(&ks_cnt), 256 * sizeof(int)));
    FAV_HIP(hipMemset(ks_cnt, 0, 256 * sizeof(int)));
    FAV_HIP(hipHostMalloc(reinterpret_cast<void**>(&sk_err_host), sizeof(unsigned), hipHostMallocMapped));
    *sk_err_host = 0;
    FAV_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&sk_err_dev), sk_err_host, 0));
    return FAV_OK;
}

int fav_net::alloc(size_t bytes, float** out)
{
    bytes = (bytes + 255) / 256 * 256;
    if (cursor < bufs.size()) {
        if (bufs[cursor].bytes < bytes) { set_error("internal: activation arena mismatch"); return FAV_EINVAL; }
        *out = static_cast<float*>(bufs[cursor++].p);
        return FAV_OK;
    }
    if (slab_left < bytes) {
        const size_t sz = std::max(bytes, (size_t)256 << 20);
        void* sp = nullptr;
        FAV_HIP(hipMalloc(&sp, sz));
        slabs.push_back(sp); slab_cur = static_cast<char*>(sp); slab_left = sz;
    }
    DevBuf b; b.bytes = bytes; b.p = slab_cur;
    slab_cur += bytes; slab_left -= bytes;
    bufs.push_back(b); ++cursor;
    *out = static_cast<float*>(b.p);
    return FAV_OK;
}

int fav_net::timed_conv(const ConvLaunch& c, int conv_index, const Layer& L, ConvKernel kernel, int* counts)
{
    if (c.pre.acc1 != nullptr && kernel != CK_WINO4) { set_error("internal: accumulator-form InstanceNorm in front of a kernel that cannot take it"); return FAV_EINVAL; }
    ConvLaunch cs = c;
    cs.reserve_cus = reserve_cus;
    cs.no_sk = shared_device ? 1 : 0;
    cs.sk_ws = sk_ws; cs.sk_flags = sk_flags; cs.sk_epoch = ++sk_epoch;      // launches of one net are stream-ordered
    cs.sk_err = sk_err_dev;
    cs.ks_ws = ks_ws; cs.ks_cnt = ks_cnt;
    if (sk_epoch == 0xffffffffu) sk_epoch = 0;
    // generic kernel while look-ahead masks are in flight: its stream-K hand-off assumes that all blocks are resident at once, and the
    // side queues' kernels land on any CU -- owners then wait for blocks that have not started (d128: 186 us against 115 us alone,
    // profiles/r02p_4arg_kernel_stats.csv).  Data-parallel grids do not wait for anybody.  The halo-resident 3x3 kernel (bf16 fast
    // mode, FAV_NO_WINO) hands tiles over the same way and takes the same descriptor.
    ConvLaunch cg = cs;
    if (reserve_cus > 0 && tuning().side_sk != 1) cg.no_sk = 1;
    auto go = [&]() { return launch_selected(kernel, cs, cg, convs[conv_index], L.cin, counts, st); };
    char tag[96] = "";
    if (TraceRange::enabled()) snprintf(tag, sizeof tag, "fav:conv%d k%d s%d %d->%d %dx%d", conv_index, L.k, L.stride, L.cin, L.cout, c.OW, c.OH);
    TraceRange tr(tag);
    if (!profiling) return go();
    ProfRec r; r.conv = conv_index;
    // (no system-scope fence at the event: the default one flushes the caches around every timed kernel -- 6 us on either side of each
    // convolution in the rocprofv3 trace, 0.18 ms per 1280x720 frame)
    FAV_HIP(hipEventCreateWithFlags(&r.a, hipEventDisableSystemFence)); FAV_HIP(hipEventCreateWithFlags(&r.b, hipEventDisableSystemFence));
    FAV_HIP(hipEventRecord(r.a, st));
    int rc = go();
    FAV_HIP(hipEventRecord(r.b, st));
    prof_pending.push_back(r);
    if ((int)prof_ms.size() <= conv_index) { prof_ms.resize(conv_index + 1, 0.0); prof_macs.resize(conv_index + 1, 0.0); prof_n.resize(conv_index + 1, 0); prof_tile.resize(conv_index + 1, 0); }
    prof_macs[conv_index] = (double)c.OH * c.OW * L.cout * L.cin * L.k * L.k;      // useful MACs only
    if (L.transposed) prof_macs[conv_index] /= (double)(L.stride * L.stride);       // (every output pixel meets k^2 / s^2 taps)
    prof_tile[conv_index] = conv_facts(kernel, c.OH, c.OW, c.COUTp, precision, c.join_skip != nullptr, L.stride).id;
    return rc;
}

static int count_convs(const std::vector<Layer>& ls)
{
    int n = 0;
    for (const Layer& l : ls) { if (l.type == L_CONV) ++n; else if (l.type == L_RES) n += count_convs(l.block); }
    return n;
}

// conv - InstanceNorm - ReLU - conv with both convolutions on the F(4x4) kernel (the first half of a residual branch,
// models_video.lua:10-39): the first convolution adds its units' statistics to the InstanceNorm's accumulators and the second forms
// scale / shift from them in its prologue -- no in_finalize launch between the two (round 5).  ls[li] = the first convolution;
// conv_cursor already points at the second one's weights
bool fav_net::acc_stats_ok(const std::vector<Layer>& ls, size_t li) const
{
    if (tuning().no_acc_stats) return false;
    if (li + 3 >= ls.size() || ls[li + 1].type != L_IN || ls[li + 2].type != L_RELU || ls[li + 3].type != L_CONV) return false;
    if (conv_cursor >= convs.size()) return false;
    const Layer& c2 = ls[li + 3]; const DevConvW& d2 = convs[conv_cursor];
    return select_conv(c2, d2, 1, 0, precision, false, 0, 0, tuning()) == CK_WINO4;      // (behind the InstanceNorm + ReLU: one pending stage)
}

// conv - InstanceNorm - ReLU - conv - InstanceNorm (models_video.lua:10-39) with both convolutions on the Winograd kernel
bool fav_net::res_block_is_winograd(const Layer& R, size_t first_conv) const
{
    const std::vector<Layer>& b = R.block;
    if (b.size() != 5 || b[0].type != L_CONV || b[1].type != L_IN || b[2].type != L_RELU || b[3].type != L_CONV || b[4].type != L_IN) return false;
    if (first_conv + 1 >= convs.size()) return false;
    for (int k = 0; k < 2; ++k) {
        const Layer& c = b[k ? 3 : 0]; const DevConvW& d = convs[first_conv + (size_t)k];
        const ConvKernel kernel = select_conv(c, d, 1, 0, precision, false, 0, 0, tuning());
        // (a pending join is for one group of 128 filters, F(4x4) included: the layers that have the F(2x2) weights as well)
        if ((kernel != CK_WINO && kernel != CK_WINO4) || d.packed[CK_WINO] == nullptr) return false;
    }
    return true;
}

int fav_net::run(std::vector<Layer>& ls, Act& cur, bool top, float* out_planar, float* out_raw)
{
    for (size_t li = 0; li < ls.size(); ++li) {
        Layer& L = ls[li];
        switch (L.type) {
        case L_PAD: {
            if (top && li == 0 && pad_folded) break;        // folded into the input assembly (upload())
            if (cur.data == nullptr || cur.join_skip != nullptr) { set_error("network: misplaced padding layer"); return FAV_EUNSUPPORTED; }
            // reflection needs pad < size on each axis (nn.SpatialReflectionPadding asserts the same)
            if (L.pad_mode == 0 && (std::max(L.pl, L.pr) >= cur.W() || std::max(L.pt, L.pb) >= cur.H())) { set_error("network: reflection padding %d %d %d %d of a %dx%d tensor", L.pl, L.pr, L.pt, L.pb, cur.W(), cur.H()); return FAV_EINVAL; }
            // index map only: a pending per-channel transform (InstanceNorm / ReLU) commutes with it and stays pending
            Act nxt;
            nxt.Hp = cur.H() + L.pt + L.pb; nxt.Wp = cur.W() + L.pl + L.pr; nxt.C = cur.C; nxt.pre = cur.pre;
            if (nxt.pre.acc1 != nullptr) { set_error("internal: accumulator-form InstanceNorm in front of a padding layer"); return FAV_EINVAL; }
            int rc = alloc((size_t)nxt.Hp * nxt.Wp * nxt.C * sizeof(float), &nxt.data); if (rc) return rc;
            rc = launch_pad_nhwc(cur.data, cur.Hp, cur.Wp, cur.P(), cur.C, cur.ups, nxt.data, L.pl, L.pr, L.pt, L.pb, L.pad_mode, st); if (rc) return rc;
            cur = nxt;
            break;
        }
        case L_CONV: {
            const DevConvW& d = convs[conv_cursor++];
            if (cur.C != d.cinp) { set_error("internal: channel pitch mismatch (%d vs %d)", cur.C, d.cinp); return FAV_EINVAL; }
            ConvLaunch c;
            c.in = cur.data; c.IH = cur.H(); c.IW = cur.W(); c.IWp = cur.P(); c.ups = cur.ups; c.CIN = d.cinp;
            c.pre = cur.pre;
            c.wgt = d.wgt; c.bias = d.bias; c.COUT = L.cout; c.COUTp = d.coutp; c.KH = c.KW = L.k; c.stride = L.stride;
            c.pad = L.pad; c.Kpad = d.kpad;
            bool has_tanh = false; float mul = 1.f;
            const bool is_final = top && only_tail(ls, li + 1, has_tanh, mul) && has_tanh && L.cout == 3;
            if (L.transposed) {
                if (cur.ups != 0) { set_error("network: SpatialFullConvolution directly after an upsampling is unsupported"); return FAV_EUNSUPPORTED; }
                if (is_final) { set_error("network: a transposed convolution as the last layer is unsupported"); return FAV_EUNSUPPORTED; }
            }
            const ConvKernel kernel = select_conv(L, d, cur.pre.stages, cur.ups, precision, is_final, c.IH, c.IW, tuning());
            if (L.transposed && kernel == CK_TCONV) {
                // by output phase on the physical input (kernels_tconv.hip): the module's own geometry
                c.OH = (c.IH - 1) * L.stride - 2 * L.pad + L.k + L.adj; c.OW = (c.IW - 1) * L.stride - 2 * L.pad + L.k + L.adj;
                if (c.OH < 1 || c.OW < 1) { set_error("network: input too small for the architecture"); return FAV_EINVAL; }
            } else if (L.transposed) {
                // stride-2 transposed convolution = stride-1 convolution over the zero-stuffed input (size 2*in with adj 1): FAV_NO_TCONV, or
                // a layer the phase kernel does not take (upload_layers lets nothing else through)
                if (L.stride != 2 || L.adj != 1 || d.wgt == nullptr) { set_error("internal: zero-stuffed SpatialFullConvolution with s=%d adj=%d", L.stride, L.adj); return FAV_EINVAL; }
                c.ups = 1; c.stuff = 1; c.IH = 2 * cur.Hp; c.IW = 2 * cur.Wp; c.stride = 1; c.pad = L.k - 1 - L.pad;
                c.OH = c.IH + 2 * c.pad - L.k + 1; c.OW = c.IW + 2 * c.pad - L.k + 1;
            } else {
                c.OH = (c.IH + 2 * L.pad - L.k) / L.stride + 1;
                c.OW = (c.IW + 2 * L.pad - L.k) / L.stride + 1;
            }
            if (kernel != CK_TCONV && (c.IH + 2 * c.pad < L.k || c.IW + 2 * c.pad < L.k)) { set_error("network: input too small for the architecture"); return FAV_EINVAL; }
            Act nxt;
            nxt.Hp = c.OH; nxt.Wp = c.OW; nxt.C = L.cout;
            if (is_final) {
                c.final_mode = 1; c.tanh_mul = mul; c.out_planar = out_planar; c.out_raw_nchw = out_raw;
                int rc = timed_conv(c, (int)conv_cursor - 1, L, kernel, nullptr); if (rc) return rc;
                cur = nxt;
                return FAV_OK;        // Tanh / MulConstant / TotalVariation are folded into the epilogue
            }
            if (L.cout % 4 != 0) { set_error("network: %d output channels (must be a multiple of 4 except for the last layer)", L.cout); return FAV_EUNSUPPORTED; }
            const bool pitched_out = lazy.active && (int)conv_cursor - 1 == lazy.conv_index;
            int rc;
            if (pitched_out) {
                // the output of a block whose join stays pending: pixel (i, j) at the linear index of the skip's pixel (i + shave, j + shave)
                if (c.OH != lazy.rows - 2 * lazy.shave || c.OW > lazy.pitch - 2 * lazy.shave) { set_error("internal: pending residual join of mismatching shapes"); return FAV_EINVAL; }
                float* base = nullptr;
                rc = alloc((size_t)lazy.rows * lazy.pitch * L.cout * sizeof(float), &base); if (rc) return rc;
                nxt.data = base + ((size_t)lazy.shave * lazy.pitch + lazy.shave) * L.cout; nxt.pitch = lazy.pitch; c.OWp = lazy.pitch;
            } else { rc = alloc((size_t)c.OH * c.OW * L.cout * sizeof(float), &nxt.data); if (rc) return rc; }
            const bool want_stats = li + 1 < ls.size() && ls[li + 1].type == L_IN;
            const ConvFacts facts = conv_facts(kernel, c.OH, c.OW, d.coutp, precision, cur.join_skip != nullptr, L.stride);
            nxt.mblocks = facts.tiles; nxt.ppitch = d.coutp;
            const bool acc = kernel == CK_WINO4 && want_stats && !pitched_out && cur.join_skip == nullptr &&
                             (acc_stats_ok(ls, li) || (branch_tail_acc_ok && !top && li + 2 == ls.size() && !tuning().no_acc_stats && precision == 0));
            if (acc) {
                DevIN& din = ins[in_cursor];                   // the InstanceNorm that follows
                nxt.acc = din.acc + (size_t)acc_parity * stat_acc_words(L.cout); nxt.acc_other = din.acc + (size_t)(acc_parity ^ 1) * stat_acc_words(L.cout);
                c.stat_acc = nxt.acc;
            }
            if (want_stats && !acc) { rc = alloc((size_t)nxt.mblocks * d.coutp * 2 * sizeof(float), &nxt.partials); if (rc) return rc; }
            if (want_stats && !acc && facts.counts) { float* cp = nullptr; rc = alloc((size_t)nxt.mblocks * sizeof(int), &cp); if (rc) return rc; nxt.counts = reinterpret_cast<int*>(cp); }
            c.out = nxt.data; c.partials = nxt.partials;
            if (cur.join_skip != nullptr || pitched_out) {
                if (kernel != CK_WINO && kernel != CK_WINO4) { set_error("internal: a pending residual join next to a convolution that is not the Winograd kernel's"); return FAV_EINVAL; }
                c.join_skip = cur.join_skip; c.join_out = cur.join_out;
            }
            if (kernel == CK_HALO3 && precision == 1) c.wgt16 = d.wgt16;
            int* counts = facts.counts ? (nxt.counts ? nxt.counts : reinterpret_cast<int*>(zeros)) : nullptr;
            rc = timed_conv(c, (int)conv_cursor - 1, L, kernel, counts); if (rc) return rc;
            cur = nxt;
            break;
        }
        case L_IN: {
            const DevIN& d = ins[in_cursor++];
            const int C = (int)L.gamma.size();
            const int M = cur.Hp * cur.Wp;
            if (cur.data == nullptr || C != cur.C) { set_error("network: misplaced InstanceNormalization"); return FAV_EUNSUPPORTED; }
            if (cur.acc != nullptr && cur.pre.stages == 0) {
                // nothing is launched: the consuming convolution forms scale / shift from the accumulators (acc_stats_ok)
                cur.pre = Affine();
                cur.pre.acc1 = cur.acc; cur.pre.acc1_zero = cur.acc_other; cur.pre.gamma1 = d.gamma; cur.pre.beta1 = d.beta; cur.pre.eps1 = L.eps; cur.pre.count1 = M;
                cur.pre.relu1 = 0; cur.pre.stages = 1;
            } else if (cur.partials != nullptr && cur.pre.stages == 0) {
                int rc = launch_in_finalize(cur.partials, cur.counts, cur.mblocks, M, CONV_BM, C, cur.ppitch, d.gamma, d.beta, L.eps,
                                            d.scale, d.shift, st);
                if (rc) return rc;
                rc = append_stage(cur.pre, d.scale, d.shift, 0); if (rc) return rc;
            } else {
                Affine normalised = cur.pre;
                int rc = append_stage(normalised, d.scale, d.shift, 0); if (rc) return rc;
                // statistics of the pending-transformed tensor (nearest upsampling replicates every
                // element s*s times and leaves mean and biased variance unchanged)
                float* part = nullptr;
                const int mb = (M + 127) / 128;
                rc = alloc((size_t)mb * C * 2 * sizeof(float), &part); if (rc) return rc;
                rc = launch_stats(cur.data, M, C, cur.pre, part, st); if (rc) return rc;
                rc = launch_in_finalize(part, nullptr, mb, M, 128, C, C, d.gamma, d.beta, L.eps, d.scale, d.shift, st); if (rc) return rc;
                cur.pre = normalised;
            }
            cur.partials = nullptr; cur.counts = nullptr; cur.acc = nullptr; cur.acc_other = nullptr;
            break;
        }
        case L_BN: {
            const DevIN& d = ins[in_cursor++];
            if (cur.data == nullptr || (int)L.mean.size() != cur.C) { set_error("network: misplaced SpatialBatchNormalization"); return FAV_EUNSUPPORTED; }
            int rc = append_stage(cur.pre, d.scale, d.shift, 0); if (rc) return rc;
            cur.partials = nullptr; cur.counts = nullptr;
            break;
        }
        case L_RELU:
            if (cur.pre.stages == 0) (void)append_stage(cur.pre, ones, zeros, 1);
            else if (cur.pre.stages == 1) cur.pre.relu1 = 1;
            else cur.pre.relu2 = 1;
            cur.partials = nullptr;
            break;
        case L_UP:
            if (L.scale != 2 || cur.ups != 0) { set_error("network: only a single x2 nearest upsampling per convolution is supported"); return FAV_EUNSUPPORTED; }
            cur.ups = 1;
            break;
        case L_RES: {
            if (cur.ups != 0) { set_error("network: residual block directly after an upsampling is unsupported"); return FAV_EUNSUPPORTED; }
            Act skip = cur;
            Act br = cur;
            br.partials = nullptr;
            int rc;
            if (cur.join_skip != nullptr) {
                // the previous block's join is pending: this block's first convolution forms it while staging its input and writes it
                // out -- that tensor is this block's skip
                float* zb = nullptr;
                rc = alloc((size_t)cur.Hp * cur.P() * cur.C * sizeof(float), &zb); if (rc) return rc;
                br.join_out = zb;
                skip = Act(); skip.data = zb; skip.Hp = cur.Hp; skip.Wp = cur.Wp; skip.C = cur.C; skip.pitch = cur.P();
            }
            // Leave THIS block's join pending when the next layer is another residual block that starts with a Winograd convolution
            // (models_video.lua:41-53, R128 x 5): the 15 us res_add launch (88 MB at the HBM roofline) becomes 33 MB of extra reads and
            // 33 MB of writes inside a kernel that is bound by its matrix instructions.  The skip must be a plain tensor (the first
            // block's skip still carries d128's InstanceNorm + ReLU: its join stays a launch).
            // Since round 4 only with the F(2x2) kernels (FAV_WINO_F2), or on request (FAV_LAZY_JOIN): inside the F(4x4) kernel the joined
            // rows' stores cost 10 us of its K loop (the weight ring runs dry behind them) on top of 8 us of staging -- more than the
            // 16 us launch they replace (639 against 634 frames/s, profiles/r4s_stream_k_and_joins_ab.log).  (The F(4x4) kernel's pending-join
            // instantiation is kept for FAV_LAZY_JOIN and the tests that pin its bits against the launched joins; since the row requests carry
            // their own offsets it spills inside its K loop -- nobody tuned it further)
            const int nconv = count_convs(L.block);
            const bool lazy_out = !tuning().no_lazy_join && (tuning().wino_f2 || tuning().lazy_join) && precision == 0 &&
                                  li + 1 < ls.size() && ls[li + 1].type == L_RES && skip.pre.stages == 0 && skip.ups == 0 &&
                                  res_block_is_winograd(L, conv_cursor) && res_block_is_winograd(ls[li + 1], conv_cursor + (size_t)nconv);
            if (lazy_out) { lazy.active = true; lazy.pitch = skip.P(); lazy.rows = skip.Hp; lazy.shave = L.shave; lazy.conv_index = (int)conv_cursor + nconv - 1; }
            // the join feeds an InstanceNorm (directly, or through the x2 nearest upsample of models_video.lua:94-98, which leaves
            // mean and biased variance unchanged): it takes that norm's statistics in the same pass
            size_t nx = li + 1;
            if (nx < ls.size() && ls[nx].type == L_UP && ls[nx].scale == 2) ++nx;
            const bool join_stats = nx < ls.size() && ls[nx].type == L_IN;
            // else, when the join is a plain res_add launch (not left pending either), it can take the branch's last InstanceNorm as
            // accumulators (round 5) -- no in_finalize launch between the branch's last convolution and the join
            branch_tail_acc_ok = !lazy_out && !join_stats;
            rc = run(L.block, br, false, nullptr, nullptr);
            lazy.active = false; branch_tail_acc_ok = false;
            if (rc) return rc;
            if (br.pre.stages != 1 || br.pre.relu1 || br.ups != 0) { set_error("network: residual branch must end in conv + InstanceNormalization"); return FAV_EUNSUPPORTED; }
            if (br.Hp != skip.Hp - 2 * L.shave || br.Wp != skip.Wp - 2 * L.shave || br.C != skip.C) {
                set_error("network: residual branch output %dx%d does not match the shaved skip %dx%d", br.Wp, br.Hp,
                          skip.Wp - 2 * L.shave, skip.Hp - 2 * L.shave);
                return FAV_EUNSUPPORTED; }
            if (lazy_out) {
                // nothing is launched: data = the branch's output (laid out under the skip), pre = its InstanceNorm, plus the skip
                cur = br;
                cur.partials = nullptr; cur.counts = nullptr;
                cur.join_skip = skip.data + ((size_t)L.shave * skip.P() + L.shave) * skip.C; cur.join_out = nullptr;
                break;
            }
            Act z; z.Hp = br.Hp; z.Wp = br.Wp; z.C = br.C;
            rc = alloc((size_t)z.Hp * z.Wp * z.C * sizeof(float), &z.data); if (rc) return rc;
            if (join_stats) {
                z.mblocks = res_add_stat_blocks(z.Hp, z.Wp); z.ppitch = z.C;
                rc = alloc((size_t)z.mblocks * z.C * 2 * sizeof(float), &z.partials); if (rc) return rc;
                float* cp = nullptr; rc = alloc((size_t)z.mblocks * sizeof(int), &cp); if (rc) return rc; z.counts = reinterpret_cast<int*>(cp);
            }
            rc = launch_res_add(br.data, br.pre.scale1, br.pre.shift1, skip.data, skip.Hp, skip.Wp, L.shave, skip.pre, z.C,
                                z.data, z.partials, z.counts, st, skip.P(), &br.pre);
            if (rc) return rc;
            cur = z;
            break;
        }
        case L_TANH: case L_MUL:
            set_error("network: Tanh/MulConstant are only supported after the last convolution"); return FAV_EUNSUPPORTED;
        case L_IDENTITY: break;
        }
    }
    if (top) { set_error("network: the model does not end in a 3-channel convolution followed by Tanh"); return FAV_EUNSUPPORTED; }
    return FAV_OK;
}

void fav_net::out_size(int H, int W, int* Ho, int* Wo) const
{
    // shape walk (models_video.lua:55-140): convs floor((in+2p-k)/s)+1, residual blocks shave, upsampling doubles
    int h = H + 2 * pad, w = W + 2 * pad;
    std::function<void(const std::vector<Layer>&)> walk = [&](const std::vector<Layer>& ls) {
        for (const Layer& L : ls) {
            if (L.type == L_PAD) { if (&L == &layers[0] && pad_folded) continue; h += L.pt + L.pb; w += L.pl + L.pr; }
            else if (L.type == L_CONV && L.transposed) { h = (h - 1) * L.stride - 2 * L.pad + L.k + L.adj; w = (w - 1) * L.stride - 2 * L.pad + L.k + L.adj; }
            else if (L.type == L_CONV) { h = (h + 2 * L.pad - L.k) / L.stride + 1; w = (w + 2 * L.pad - L.k) / L.stride + 1; }
            else if (L.type == L_UP) { h *= L.scale; w *= L.scale; }
            else if (L.type == L_RES) walk(L.block);
        }
    };
    walk(layers);
    *Ho = h; *Wo = w;
}

// The persistent / stream-K convolution grids assume that the forwards of ONE process on a device do not overlap (fav.h, concurrency
// note).  Forwards enqueued on different HIP streams -- two networks, or one network driven from two streams -- used to be a
// documented foot-gun; now the library orders them itself: when a forward arrives on another stream than the previous forward on
// that device, the HOST first waits for the previous stream to drain (hipStreamSynchronize: rare, a misuse made safe).  No marker
// is left in the compute queue in the common single-stream case: on this runtime an event record behind long-running kernels keeps
// a runtime thread spinning until it fires (scripts/runtime_thread_bench.hip).  Other PROCESSES on the device remain the caller's
// business (fav_net_set_shared_device).
namespace {
struct DeviceOrder { std::mutex mu; hipStream_t last = nullptr; bool valid = false; };
DeviceOrder& device_order(int device)
{
    static DeviceOrder order[64];
    return order[(device >= 0 && device < 64) ? device : 0];
}
}  // namespace

// the owner of `stream` is about to destroy it: drain it while the handle is still valid and forget it, so that the next forward
// never synchronises a dead (or recycled) handle
static void forget_stream(int device, hipStream_t stream)
{
    DeviceOrder& ord = device_order(device);
    std::lock_guard<std::mutex> order_lock(ord.mu);
    if (ord.valid && ord.last == stream) { (void)hipStreamSynchronize(stream); ord.valid = false; ord.last = nullptr; }
}

extern "C" int fav_net_forget_stream(fav_net* net, fav_hipstream_t stream)
{
    FAV_REQUIRE(net, "fav_net_forget_stream: null network");
    FAV_HIP(hipSetDevice(net->device));
    forget_stream(net->device, static_cast<hipStream_t>(stream));
    return FAV_OK;
}

int fav_net::forward_padded(const float* in8, int H, int W, float* out_planar, float* out_raw, hipStream_t stream)
{
    FAV_HIP(hipSetDevice(device));
    DeviceOrder& ord = device_order(device);
    std::lock_guard<std::mutex> order_lock(ord.mu);       // (handles are not thread-safe; this only keeps the bookkeeping consistent)
    if (ord.valid && ord.last != stream && hipStreamSynchronize(ord.last) != hipSuccess)
        (void)hipGetLastError();       // (a handle destroyed without fav_net_forget_stream / destroying its frame pipeline first: fav.h asks for either)
    ord.valid = true; ord.last = stream;
    return forward_padded_unordered(in8, H, W, out_planar, out_raw, stream);
}

int fav_net::forward_padded_unordered(const float* in8, int H, int W, float* out_planar, float* out_raw, hipStream_t stream)
{
    if (sk_err_host && *reinterpret_cast<volatile unsigned*>(sk_err_host)) {      // reported by an earlier launch of this net
        *sk_err_host = 0;
        shared_device = true;
        set_error("a stream-K hand-off between convolution blocks timed out in an earlier launch of this network: its result was "
                  "wrong (two networks running concurrently on one device? see the concurrency note in fav.h)");
        return FAV_EHIP;
    }
    if (H != curH || W != curW) {
        if (!bufs.empty()) {
            FAV_HIP(hipDeviceSynchronize());
            for (void* sp : slabs) (void)hipFree(sp);
            slabs.clear(); slab_cur = nullptr; slab_left = 0;
            bufs.clear();
        }
        curH = H; curW = W;
    }
    st = stream; cursor = 0; conv_cursor = 0; in_cursor = 0;
    // InstanceNorm accumulators (Affine::acc1): a forward adds to one half and its consumers zero the other for the next one.  The halves
    // alternate over the forwards that USE them (fp32 mode; which layers do depends on the network and the process-wide switches only), so a
    // half is zero whenever it is added to -- unless a forward stopped between a producer and its consumer: then everything is zeroed here
    if (acc_dirty) {
        for (DevIN& i : ins) if (i.acc) FAV_HIP(hipMemsetAsync(i.acc, 0, i.acc_bytes, stream));
        acc_dirty = false;
    }
    if (precision == 0 && !tuning().no_acc_stats && !tuning().no_wino) acc_parity ^= 1;
    Act cur;
    cur.data = const_cast<float*>(in8); cur.Hp = H + 2 * pad; cur.Wp = W + 2 * pad; cur.C = 8;
    const int rc = run(exec, cur, true, out_planar, out_raw);
    if (rc) acc_dirty = true;
    return rc;
}

// ================================================================================================
// C ABI: network
// ================================================================================================
static int finish_create(fav_net* net, fav_net** out)
{
    int rc = net->upload();
    if (rc) { delete net; return rc; }
    *out = net;
    return FAV_OK;
}

extern "C" int fav_net_create(const char* t7_path_host, int device, fav_net** out)
{
    FAV_REQUIRE(t7_path_host && out, "fav_net_create: null argument");
    int rc = ensure_device(); if (rc) return rc;
    FAV_ABI_TRY
    std::unique_ptr<fav_net> net(new fav_net());
    net->device = device;
    rc = t7_parse_model(t7_path_host, net->layers);
    if (rc) return rc;
    return finish_create(net.release(), out);
    FAV_ABI_CATCH("fav_net_create")
}

extern "C" int fav_net_pack_host(const char* t7_path_host, void* blob_host, size_t capacity, size_t* bytes)
{
    FAV_REQUIRE(t7_path_host && bytes, "fav_net_pack_host: null argument");
    FAV_ABI_TRY
    std::vector<Layer> layers;
    int rc = t7_parse_model(t7_path_host, layers); if (rc) return rc;
    std::vector<uint8_t> blob;
    rc = blob_pack(layers, blob); if (rc) return rc;
    *bytes = blob.size();
    if (blob_host) {
        FAV_REQUIRE(capacity >= blob.size(), "fav_net_pack_host: capacity %zu < %zu", capacity, blob.size());
        memcpy(blob_host, blob.data(), blob.size());
    }
    return FAV_OK;
    FAV_ABI_CATCH("fav_net_pack_host")
}

extern "C" int fav_net_create_from_blob(const void* blob_host, size_t bytes, int device, fav_net** out)
{
    FAV_REQUIRE(blob_host && out, "fav_net_create_from_blob: null argument");
    int rc = ensure_device(); if (rc) return rc;
    FAV_ABI_TRY
    std::unique_ptr<fav_net> net(new fav_net());
    net->device = device;
    rc = blob_unpack(blob_host, bytes, net->layers);
    if (rc) return rc;
    return finish_create(net.release(), out);
    FAV_ABI_CATCH("fav_net_create_from_blob")
}

extern "C" void fav_net_destroy(fav_net* net) { delete net; }

extern "C" int fav_net_check(fav_net* net)
{
    FAV_REQUIRE(net, "fav_net_check: null net");
    if (net->sk_err_host && *reinterpret_cast<volatile unsigned*>(net->sk_err_host)) {
        *net->sk_err_host = 0;
        net->shared_device = true;      // from now on: data-parallel grids, which need no co-resident blocks
        set_error("a stream-K hand-off between convolution blocks timed out: the frame(s) computed since the last check are wrong "
                  "(another context holding compute units of this device? see the concurrency note in fav.h); this network now runs "
                  "with data-parallel grids (fav_net_set_shared_device)");
        return FAV_EHIP;
    }
    return FAV_OK;
}

extern "C" int fav_net_set_shared_device(fav_net* net, int shared)
{
    FAV_REQUIRE(net, "fav_net_set_shared_device: null net");
    net->shared_device = shared != 0;
    return FAV_OK;
}

extern "C" int fav_net_describe_host(const fav_net* net, char* buf_host, size_t capacity)
{
    FAV_REQUIRE(net && buf_host && capacity > 0, "fav_net_describe_host: null argument");
    const std::string s = describe_layers(net->layers);
    FAV_REQUIRE(s.size() + 1 <= capacity, "fav_net_describe_host: need %zu bytes", s.size() + 1);
    memcpy(buf_host, s.c_str(), s.size() + 1);
    return FAV_OK;
}

extern "C" int fav_net_profile_enable(fav_net* net, int on)
{
    FAV_REQUIRE(net, "fav_net_profile_enable: null net");
    net->profiling = on != 0;
    return FAV_OK;
}

extern "C" int fav_net_profile_read_host(fav_net* net, int capacity, int* count, double* ms_sum, int* launches,
                                         double* macs_per_launch, int* ntile)
{
    FAV_REQUIRE(net && count && ms_sum && launches && macs_per_launch && ntile, "fav_net_profile_read_host: null argument");
    FAV_HIP(hipSetDevice(net->device));
    for (auto& r : net->prof_pending) {
        FAV_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        FAV_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        net->prof_ms[r.conv] += ms; net->prof_n[r.conv] += 1;
        (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
    }
    net->prof_pending.clear();
    const int n = (int)net->prof_ms.size();
    FAV_REQUIRE(n <= capacity, "fav_net_profile_read_host: need capacity %d", n);
    for (int i = 0; i < n; ++i) { ms_sum[i] = net->prof_ms[i]; launches[i] = net->prof_n[i]; macs_per_launch[i] = net->prof_macs[i]; ntile[i] = net->prof_tile[i]; }
    *count = n;
    std::fill(net->prof_ms.begin(), net->prof_ms.end(), 0.0); std::fill(net->prof_n.begin(), net->prof_n.end(), 0);
    return FAV_OK;
}

extern "C" int fav_t7_describe_host(const char* t7_path_host, char* buf_host, size_t capacity)
{
    FAV_REQUIRE(t7_path_host && buf_host && capacity > 0, "fav_t7_describe_host: null argument");
    FAV_ABI_TRY
    std::vector<Layer> layers;
    int rc = t7_parse_model(t7_path_host, layers); if (rc) return rc;
    const std::string s = describe_layers(layers);
    FAV_REQUIRE(s.size() + 1 <= capacity, "fav_t7_describe_host: need %zu bytes", s.size() + 1);
    memcpy(buf_host, s.c_str(), s.size() + 1);
    return FAV_OK;
    FAV_ABI_CATCH("fav_t7_describe_host")
}

extern "C" long long fav_net_param_count(const fav_net* net) { return net ? net->params : 0; }

extern "C" int fav_net_output_size(const fav_net* net, int H, int W, int* Ho, int* Wo)
{
    FAV_REQUIRE(net && Ho && Wo && H > 0 && W > 0, "fav_net_output_size: bad argument");
    net->out_size(H, W, Ho, Wo);
    return FAV_OK;
}

extern "C" int fav_net_forward(fav_net* net, const float* in7, float* out3, int H, int W, fav_hipstream_t stream)
{
    FAV_REQUIRE(net && in7 && out3 && H > 0 && W > 0, "fav_net_forward: bad argument");
    FAV_REQUIRE(net->pad < H && net->pad < W, "fav_net_forward: %dx%d is smaller than the reflection padding %d", W, H, net->pad);
    FAV_HIP(hipSetDevice(net->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // boundary conversion: NCHW [7][H][W] -> reflection-padded NHWC8 (nn.SpatialReflectionPadding folded in)
    const size_t bytes = (size_t)(H + 2 * net->pad) * (W + 2 * net->pad) * 8 * sizeof(float);
    if (net->stage_bytes < bytes) {
        FAV_HIP(hipDeviceSynchronize());
        (void)hipFree(net->stage); net->stage = nullptr; net->stage_bytes = 0;
        FAV_HIP(hipMalloc(reinterpret_cast<void**>(&net->stage), bytes));
        net->stage_bytes = bytes;
    }
    float* in8 = net->stage;
    int rc = launch_nchw_to_nhwc_pad(in7, net->in_channels, H, W, net->pad, 8, in8, st); if (rc) return rc;
    return net->forward_padded(in8, H, W, nullptr, out3, st);
}

// nn.SpatialConvolution [+ nn.InstanceNormalization [+ nn.ReLU]] as a stand-alone operator (tests / ops)
extern "C" int fav_conv2d_nchw_f32(const float* in, int Cin, int H, int W, const float* weight, const float* bias, int Cout,
                                   int k, int stride, int pad, const float* gamma, const float* beta, float eps, int relu,
                                   float* out, fav_hipstream_t stream)
{
    FAV_REQUIRE(in && weight && out && Cin > 0 && Cout > 0 && k > 0 && stride > 0 && pad >= 0, "fav_conv2d_nchw_f32: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int cinp = (Cin + 3) / 4 * 4, coutp = (Cout + 31) / 32 * 32, kpad = (k * k * cinp + 31) / 32 * 32;
    const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
    FAV_REQUIRE(OH > 0 && OW > 0, "fav_conv2d_nchw_f32: empty output");
    const int M = OH * OW, mb = conv_mblocks(OH, OW);
    Layer L; L.cin = Cin; L.cout = Cout; L.k = k;
    L.w.resize((size_t)Cin * Cout * k * k);
    FAV_HIP(hipMemcpy(L.w.data(), weight, L.w.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<float> wre, hb((size_t)coutp, 0.f);
    repack_weights(L, cinp, coutp, kpad, wre);
    if (bias) FAV_HIP(hipMemcpy(hb.data(), bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToHost));
    float *dw = nullptr, *db = nullptr, *din = nullptr, *dout = nullptr, *dpart = nullptr, *dsc = nullptr, *dsh = nullptr;
    auto cleanup = [&]() { (void)hipFree(dw); (void)hipFree(db); (void)hipFree(din); (void)hipFree(dout); (void)hipFree(dpart); (void)hipFree(dsc); (void)hipFree(dsh); };
    rc = dev_upload(wre, 0, &dw); if (rc) { cleanup(); return rc; }
    rc = dev_upload(hb, 0, &db); if (rc) { cleanup(); return rc; }
    if (hipMalloc(reinterpret_cast<void**>(&din), (size_t)H * W * cinp * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dout), (size_t)M * Cout * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dpart), (size_t)mb * coutp * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dsc), (size_t)coutp * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dsh), (size_t)coutp * 4) != hipSuccess) { cleanup(); return hip_fail(hipErrorOutOfMemory, "hipMalloc"); }
    rc = launch_nchw_to_nhwc_pad(in, Cin, H, W, 0, cinp, din, st);
    ConvLaunch c;
    c.in = din; c.IH = H; c.IW = W; c.IWp = W; c.CIN = cinp; c.wgt = dw; c.bias = db; c.COUT = Cout; c.COUTp = coutp;
    c.KH = c.KW = k; c.stride = stride; c.pad = pad; c.Kpad = kpad; c.OH = OH; c.OW = OW; c.out = dout;
    c.partials = gamma ? dpart : nullptr;
    if (!rc) rc = launch_conv(c, st);
    Affine t;
    if (!rc && gamma) {
        rc = launch_in_finalize(dpart, nullptr, mb, M, CONV_BM, Cout, coutp, gamma, beta, eps, dsc, dsh, st);
        t.scale1 = dsc; t.shift1 = dsh; t.relu1 = relu; t.stages = 1;
    }
    if (!rc) rc = launch_nhwc_to_nchw(dout, M, Cout, t, out, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = hip_fail(hipGetLastError(), "fav_conv2d_nchw_f32");
    cleanup();
    return rc;
}

// nn.SpatialFullConvolution [+ nn.InstanceNormalization [+ nn.ReLU]] as a stand-alone operator: stride >= 2 on the phase kernel
// (kernels_tconv.hip), stride 1 as the ordinary convolution it is
extern "C" int fav_conv_transpose2d_nchw_f32(const float* in, int Cin, int H, int W, const float* weight, const float* bias, int Cout,
                                             int k, int stride, int pad, int adj, const float* gamma, const float* beta, float eps, int relu,
                                             float* out, fav_hipstream_t stream)
{
    FAV_REQUIRE(in && weight && out && Cin > 0 && Cout > 0 && H > 0 && W > 0, "fav_conv_transpose2d_nchw_f32: bad argument");
    FAV_REQUIRE(k >= 1 && k <= TCONV_MAX_K && stride >= 1 && stride <= TCONV_MAX_S && pad >= 0 && pad <= k - 1 && adj >= 0 && adj < stride,
                "fav_conv_transpose2d_nchw_f32: supported for k <= %d, stride <= %d, pad <= k - 1, adj < stride, got k=%d s=%d pad=%d adj=%d",
                TCONV_MAX_K, TCONV_MAX_S, k, stride, pad, adj);
    int rc = ensure_device(); if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::vector<float> hw((size_t)Cin * Cout * k * k);
    FAV_HIP(hipMemcpy(hw.data(), weight, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (stride == 1) {
        std::vector<float> wc;
        conv_tconv_as_conv(hw.data(), Cin, Cout, k, wc);
        float* dwc = nullptr;
        rc = dev_upload(wc, 0, &dwc);
        if (!rc) rc = fav_conv2d_nchw_f32(in, Cin, H, W, dwc, bias, Cout, k, 1, k - 1 - pad, gamma, beta, eps, relu, out, stream);
        (void)hipFree(dwc);
        return rc;
    }
    const int cinp = (Cin + 7) / 8 * 8, coutp = (Cout + 31) / 32 * 32;
    const int OH = (H - 1) * stride - 2 * pad + k + adj, OW = (W - 1) * stride - 2 * pad + k + adj;
    FAV_REQUIRE(OH > 0 && OW > 0, "fav_conv_transpose2d_nchw_f32: empty output");
    const int M = OH * OW, mb = conv_tconv_tiles(OH, OW, stride);
    std::vector<float> wpk, hb((size_t)coutp, 0.f);
    conv_tconv_pack(hw.data(), Cin, Cout, cinp, coutp, k, stride, pad, wpk);
    if (bias) FAV_HIP(hipMemcpy(hb.data(), bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToHost));      // (nothing is allocated yet)
    float *dw = nullptr, *db = nullptr, *din = nullptr, *dout = nullptr, *dpart = nullptr, *dsc = nullptr, *dsh = nullptr; int* dcnt = nullptr;
    auto cleanup = [&]() { (void)hipFree(dw); (void)hipFree(db); (void)hipFree(din); (void)hipFree(dout); (void)hipFree(dpart); (void)hipFree(dsc); (void)hipFree(dsh); (void)hipFree(dcnt); };
    rc = dev_upload(wpk, 0, &dw); if (rc) { cleanup(); return rc; }
    rc = dev_upload(hb, 0, &db); if (rc) { cleanup(); return rc; }
    if (hipMalloc(reinterpret_cast<void**>(&din), (size_t)H * W * cinp * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dout), (size_t)M * Cout * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dpart), (size_t)mb * coutp * 8) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dcnt), (size_t)mb * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dsc), (size_t)coutp * 4) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&dsh), (size_t)coutp * 4) != hipSuccess) { cleanup(); return hip_fail(hipErrorOutOfMemory, "hipMalloc"); }
    rc = launch_nchw_to_nhwc_pad(in, Cin, H, W, 0, cinp, din, st); if (rc) { cleanup(); return rc; }
    ConvLaunch c;
    c.in = din; c.IH = H; c.IW = W; c.IWp = W; c.CIN = cinp; c.bias = db; c.COUT = Cout; c.COUTp = coutp;
    c.KH = c.KW = k; c.stride = stride; c.pad = pad; c.OH = OH; c.OW = OW; c.out = dout;
    c.partials = gamma ? dpart : nullptr;
    if (!rc) rc = launch_conv_tconv(c, dw, dcnt, st);
    Affine t;
    if (!rc && gamma) {
        rc = launch_in_finalize(dpart, dcnt, mb, M, CONV_BM, Cout, coutp, gamma, beta, eps, dsc, dsh, st);
        t.scale1 = dsc; t.shift1 = dsh; t.relu1 = relu; t.stages = 1;
    }
    if (!rc) rc = launch_nhwc_to_nchw(dout, M, Cout, t, out, st);
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = hip_fail(hipGetLastError(), "fav_conv_transpose2d_nchw_f32");
    cleanup();
    return rc;
}

extern "C" int fav_net_set_precision(fav_net* net, int mode)
{
    FAV_REQUIRE(net && (mode == 0 || mode == 1), "fav_net_set_precision: mode must be FAV_PRECISION_FP32 or FAV_PRECISION_BF16_OPERANDS");
    if (net->precision != mode) { net->curH = -1; net->acc_dirty = true; }      // the two modes tile (and size the statistics buffers) differently: rebuild the arena
    net->precision = mode;
    return FAV_OK;
}

// internal accessors for the other host units (vr.cpp, stream.cpp)
namespace fav {
int net_device(const fav_net* n) { return n->device; }
int net_pad(const fav_net* n) { return n->pad; }
int net_in_channels(const fav_net* n) { return n->in_channels; }
void net_out_size(const fav_net* n, int H, int W, int* Ho, int* Wo) { n->out_size(H, W, Ho, Wo); }
int net_forward_padded(fav_net* n, const float* in8, int H, int W, float* out_planar, hipStream_t st) { return n->forward_padded(in8, H, W, out_planar, nullptr, st); }
void net_forget_stream(const fav_net* n, hipStream_t st) { forget_stream(n->device, st); }
// Only ever raised: the field is 0 or the one process-wide count the streams reserve (stream.cpp, SIDE_CUS), so max() is also the plain
// assignment of a look-ahead mask, and an asynchronous encoder never takes back what a look-ahead reserved
void net_reserve_cus(fav_net* n, int cus) { n->reserve_cus = std::max(n->reserve_cus, cus); }
}  // namespace fav
