// net_model.cpp -- from a parsed checkpoint to what fav_net runs: the executed copy of the layers (stride-1 transposed convolutions
// rewritten, channel counts padded), the one record per ConvKernel, every kernel's packing of the weights, the upload.
#include <cmath>

#include "net_internal.h"
#include "wino_pack.h"
#include "wino4_pack.h"
#include "up2_pack.h"
#include "s2_pack.h"
#include "tconv_pack.h"
#include "first_pack.h"
#include "first2d_pack.h"
#include "fold_pack.h"

namespace fav {

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

namespace {

// w: the layer's weights as the checkpoint has them ([cout][cin][k][k]; transposed: [cin][cout][k][k]), s: the layer
using Weights = std::vector<float>;
void pack_c8d(const float* w, const ConvShape& s, Weights& out) { conv_c8d_pack(w, s.cin_real, s.cout, out); }
void pack_first1d(const float* w, const ConvShape& s, Weights& out) { conv_first_pack(w, s.cin_real, s.cout, out); }
void pack_first2d(const float* w, const ConvShape& s, Weights& out)      // a first layer with more than 32 filters: groups of 32
{
    if (s.coutp == 32) conv_first2d_pack(w, s.cin_real, s.cout, out); else conv_first2d_pack_groups(w, s.cin_real, s.cout, s.coutp, out);
}
void pack_wino(const float* w, const ConvShape& s, Weights& out) { conv_wino_pack(w, s.cin_real, s.cout, out); }
void pack_wino4(const float* w, const ConvShape& s, Weights& out) { conv_wino4_pack_groups(w, s.cin_real, s.cout, out); }      // any number of 128-filter groups
void pack_up2(const float* w, const ConvShape& s, Weights& out)
{
    if (s.cout == 64) {
        Weights w9;
        conv_up2_pack(w, s.cin_real, out);
        conv_up2w_pack(w, s.cin_real, w9);                        // the nine-position form follows the phase-merged one
        out.insert(out.end(), w9.begin(), w9.end());
    } else conv_up2w_pack_groups(w, s.cin_real, s.cout, out);      // more than 64 filters: the nine-position form only, one block per group of 64
}
void pack_s2w(const float* w, const ConvShape& s, Weights& out) { conv_s2w_pack_groups(w, s.cin_real, s.cout, out); }
void pack_fold(const float* w, const ConvShape& s, Weights& out) { conv_fold_pack(w, s.cin_real, s.cin_pitch, s.cout, s.k, out); }
void pack_tconv(const float* w, const ConvShape& s, Weights& out) { conv_tconv_pack(w, s.cin_real, s.cout, s.cin_pitch, s.coutp, s.k, s.stride, s.pad, out); }

#ifdef FAV_DIAG
#define OFF(name) name
#else
#define OFF(name) nullptr      // (the release library does not even hold the switches' names: fav_internal.h, diag_env)
#endif
//   kernel      name       off switch           eligible               input state  pack          tiles               counts  id   rule            launch               hands over
constexpr ConvKernelInfo CONV_KERNEL_TABLE[CONV_KERNELS] = {
    {CK_GENERIC, "generic", nullptr,             nullptr,               IN_PLAIN,    nullptr,      conv_tiles,         false,  0,   ID_N_TILE,      launch_conv,         true},
    {CK_FOLD,    "fold",    OFF("FAV_NO_FOLD"),  conv_fold_eligible,    IN_PLAIN,    pack_fold,    nullptr,            false,  1,   ID_FIXED,       launch_conv_fold,    false},      // the row-folded last layer
    {CK_C8,      "c8",      OFF("FAV_NO_C8"),    conv_c8_eligible,      IN_PLAIN,    nullptr,      conv_c8_tiles,      true,   8,   ID_FIXED,       launch_conv_c8,      false},      // first layer, all 8 channels
    {CK_C8D,     "c8d",     OFF("FAV_NO_C8D"),   conv_c8d_eligible,     IN_PLAIN,    pack_c8d,     conv_c8_tiles,      true,   7,   ID_FIXED,       launch_conv_c8d,     false},      // ... dense-K pairing
    {CK_FIRST1D, "first1d", OFF("FAV_NO_FIRST"), conv_c8d_eligible,     IN_PLAIN,    pack_first1d, conv_first_tiles,   true,   6,   ID_FIXED,       launch_conv_first,   false},      // ... F(2,3) along x
    {CK_FIRST2D, "first2d", OFF("FAV_NO_FIRST"), conv_first2d_eligible, IN_PLAIN,    pack_first2d, conv_first2d_tiles, true,   16,  ID_FIXED,       launch_conv_first2d, false},      // ... F(2x2,3x3) over its nine 3x3 blocks
    {CK_S2W,     "s2w",     OFF("FAV_NO_S2W"),   conv3s2w_eligible,     IN_NORM,     pack_s2w,     conv3s2w_tiles,     true,   700, ID_PLUS_N,      launch_conv3s2w,     false},      // 3x3 stride 2: fragment order
    {CK_UP2,     "up2",     OFF("FAV_NO_UP2"),   conv3_up2_eligible,    IN_NORM_UP2, pack_up2,     conv3_up2_tiles,    true,   500, ID_PLUS_N,      launch_conv3_up2,    false},      // 3x3 after a x2 upsampling: merged 2x2 taps
    {CK_WINO,    "wino",    OFF("FAV_NO_WINO"),  conv3_wino_eligible,   IN_PLAIN,    pack_wino,    conv3_wino_tiles,   true,   400, ID_PLUS_N_JOIN, launch_conv3_wino,   false},      // residual 3x3: Winograd F(2x2,3x3)
    {CK_WINO4,   "wino4",   OFF("FAV_NO_WINO"),  conv3_wino4_eligible,  IN_PLAIN,    pack_wino4,   conv3_wino4_tiles,  true,   600, ID_PLUS_N_JOIN, launch_conv3_wino4,  false},      // ... as F(4x4,3x3)
    {CK_HALO3,   "halo3",   OFF("FAV_NO_H3"),    conv3_halo_eligible,   IN_PLAIN,    nullptr,      conv3_halo_tiles,   true,   300, ID_PLUS_N,      launch_conv3_halo,   true},
    {CK_S2HALO,  "s2halo",  OFF("FAV_NO_S2"),    conv3s2_eligible,      IN_NORM,     nullptr,      conv3s2_tiles,      true,   200, ID_PLUS_N,      launch_conv3s2,      true},
    {CK_TCONV,   "tconv",   OFF("FAV_NO_TCONV"), conv_tconv_eligible,   IN_PLAIN,    pack_tconv,   conv_tconv_tiles,   true,   800, ID_PLUS_N,      launch_conv_tconv,   false},      // transposed, by output phase (FAV_NO_TCONV: generic kernel, zero-stuffed input, stride 2 adj 1 only)
};
constexpr bool table_in_enum_order(int k = 0) { return k == CONV_KERNELS || (CONV_KERNEL_TABLE[k].kernel == k && table_in_enum_order(k + 1)); }
static_assert(sizeof CONV_KERNEL_TABLE / sizeof CONV_KERNEL_TABLE[0] == CONV_KERNELS && table_in_enum_order(), "one row per ConvKernel, in enum order");
#undef OFF

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

}  // namespace

const ConvKernelInfo& conv_kernel(ConvKernel k) { return CONV_KERNEL_TABLE[k]; }

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

}  // namespace fav

using namespace fav;

// n elements (zeroed on request) | h, zero-padded to pad_to elements: owned by the net, *view = the allocation
template <class T> int fav_net::dev_new(T** view, size_t n, bool zeroed)
{
    dev_ptr<T> d;
    const int rc = dev_alloc(d, n); if (rc) return rc;
    if (zeroed) FAV_HIP(hipMemset(d.get(), 0, n * sizeof(T)));
    owned.emplace_back(); owned.back().reset(*view = d.release());
    return FAV_OK;
}
template <class T> int fav_net::dev_put(T** view, const std::vector<T>& h, size_t pad_to)
{
    dev_ptr<T> d;
    const int rc = dev_upload(d, h, pad_to); if (rc) return rc;
    owned.emplace_back(); owned.back().reset(*view = d.release());
    return FAV_OK;
}

int fav_net::upload_layers(std::vector<Layer>& ls, int& chan_pitch, int& maxc)
{
    for (Layer& L : ls) {
        if (L.type == L_CONV) {
            L.dev_index = (int)convs.size();
            convs.emplace_back();
            DevConvW& d = convs.back();
            if (L.cin > chan_pitch || (chan_pitch != 8 && L.cin != chan_pitch)) {
                set_error("network: conv expects %d input channels, producer has %d", L.cin, chan_pitch); return FAV_EFORMAT; }
            if (L.k < 1 || L.stride < 1 || L.pad < 0) { set_error("network: bad convolution geometry"); return FAV_EFORMAT; }
            // channel pitches are powers of two (the generic kernel locates (tap, channel) with shifts, the elementwise kernels split 256
            // threads over the channels): 4 ... 1024 -- every architecture string of models_video.lua / train_video.lua:21-23.  Refused
            // here, at load time: a 48-channel model used to overrun the repacked weight matrix before any launch could refuse it
            if ((chan_pitch & (chan_pitch - 1)) != 0) {
                set_error("network: a convolution with %d input channels is unsupported (channel counts must be powers of two)", chan_pitch);
                return FAV_EUNSUPPORTED; }
            const ConvShape& s = d.s = {chan_pitch, L.cin, L.cout, (L.cout + 31) / 32 * 32, L.k, L.stride, L.pad, L.adj, L.transposed, 0, 0};
            d.kpad = (L.k * L.k * s.cin_pitch + 31) / 32 * 32;
            // a transposed layer runs by output phase (CK_TCONV); the zero-stuffed form on the generic kernel -- a x2 index map: stride 2,
            // adj 1 ONLY -- is what is left for a layer the phase kernel does not take (a 4-channel input pitch), and for FAV_NO_TCONV
            const bool phase = !tuning().off[CK_TCONV] && conv_tconv_eligible(s);
            if (L.transposed && !phase && (L.stride != 2 || L.adj != 1) && L.stride >= 2 && L.stride <= TCONV_MAX_S && L.k <= TCONV_MAX_K && L.pad <= L.k - 1 && L.adj >= 0 && L.adj < L.stride) {
                if (tuning().off[CK_TCONV]) set_error("network: the zero-stuffed form of SpatialFullConvolution (diagnostic switch) is stride 2, adj 1 only, got s=%d adj=%d", L.stride, L.adj);
                else set_error("network: SpatialFullConvolution with s=%d adj=%d behind %d input channels is unsupported (other than stride 2, adj 1 it needs a multiple of 8)", L.stride, L.adj, s.cin_pitch);
                return FAV_EUNSUPPORTED; }
            std::vector<float> w;
            int rc = FAV_OK;
            if (!phase) {                   // (the phase kernel reads its own packing only: no generic weight matrix for it)
                repack_weights(L, s.cin_pitch, s.coutp, d.kpad, w);
                rc = dev_put(&d.wgt, w); if (rc) return rc;
            }
            rc = dev_put(&d.bias, L.b, (size_t)s.coutp); if (rc) return rc;
            if (conv3_halo_eligible(s)) {      // bf16 copy for the fast mode (round to nearest even)
                std::vector<unsigned short> w16(w.size());
                for (size_t i = 0; i < w.size(); ++i) { unsigned b; memcpy(&b, &w[i], 4); w16[i] = (unsigned short)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16); }
                rc = dev_put(&d.wgt16, w16); if (rc) return rc;
            }
            if (L.transposed && (L.k > TCONV_MAX_K || L.stride < 2 || L.stride > TCONV_MAX_S || L.pad > L.k - 1 || L.adj < 0 || L.adj >= L.stride)) {
                set_error("network: SpatialFullConvolution is supported for k <= %d, stride <= %d, pad <= k - 1, adj < stride (models_video.lua:81-89,99-102), got k=%d s=%d pad=%d adj=%d",
                          TCONV_MAX_K, TCONV_MAX_S, L.k, L.stride, L.pad, L.adj);
                return FAV_EUNSUPPORTED; }
            // every kernel's own form of the weights, where it has one and can EVER run the layer (its input state); else packed[k] stays null
            for (const ConvKernelInfo& k : CONV_KERNEL_TABLE)
                if (k.pack && k.eligible(with_input(s, k.pack_state))) {
                    k.pack(L.w.data(), s, w);
                    rc = dev_put(&d.packed[k.kernel], w); if (rc) return rc;
                }
            chan_pitch = L.cout;
            maxc = std::max(maxc, std::max(s.coutp, s.cin_pitch));
        } else if (L.type == L_IN) {
            if ((int)L.gamma.size() != chan_pitch) { set_error("network: InstanceNormalization(%zu) after %d channels", L.gamma.size(), chan_pitch); return FAV_EFORMAT; }
            L.dev_index = (int)ins.size();
            ins.emplace_back();
            DevIN& d = ins.back();
            int rc = dev_put(&d.gamma, L.gamma); if (rc) return rc;
            rc = dev_put(&d.beta, L.beta); if (rc) return rc;
            d.acc_bytes = 2 * stat_acc_words((int)L.gamma.size()) * sizeof(long long);
            if (dev_new(&d.scale, L.gamma.size()) || dev_new(&d.shift, L.gamma.size()) || dev_new(&d.acc, d.acc_bytes / sizeof(long long), true)) return FAV_EHIP;
        } else if (L.type == L_BN) {
            if ((int)L.mean.size() != chan_pitch) { set_error("network: SpatialBatchNormalization(%zu) after %d channels", L.mean.size(), chan_pitch); return FAV_EFORMAT; }
            // evaluate mode: a fixed per-channel affine, folded into the consumer's load like InstanceNorm's
            std::vector<float> sc(L.mean.size()), sh(L.mean.size());
            for (size_t i = 0; i < sc.size(); ++i) {
                const double s = (double)L.gamma[i] / std::sqrt((double)L.var[i] + (double)L.eps);
                sc[i] = (float)s; sh[i] = (float)((double)L.beta[i] - (double)L.mean[i] * s);
            }
            L.dev_index = (int)ins.size();
            ins.emplace_back();
            DevIN& d = ins.back();
            int rc = dev_put(&d.scale, sc); if (rc) return rc;
            rc = dev_put(&d.shift, sh); if (rc) return rc;
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
    if (dev_put(&ones, o) || dev_put(&zeros, z) ||
        dev_new(&sk_ws, conv_streamk_workspace_bytes() / sizeof(float)) || dev_new(&sk_flags, (size_t)conv_streamk_grid(), true) ||
        dev_new(&ks_ws, conv3_wino4_ksplit_bytes() / sizeof(float)) || dev_new(&ks_cnt, 256, true) ||
        host_alloc(sk_err_host, 1, hipHostMallocMapped)) return FAV_EHIP;
    *sk_err_host = 0;
    FAV_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&sk_err_dev), sk_err_host.get(), 0));
    return FAV_OK;
}
