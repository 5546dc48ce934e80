// net.cpp -- host side of the transformer network (A8): kernel selection, the executor, forward ordering, fav_net's C ABI.  (The device
// form of the weights: net_model.cpp; the stand-alone operators: ops.cpp.)
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
#include <cmath>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>

#include "net_internal.h"

using namespace fav;

const Tuning& fav::tuning() { static const Tuning t; return t; }

namespace {

// Which kernel runs the convolution of shape s (weights d; s.stages / s.ups: the pending normalisations and the pending x`2^ups`
// upsampling of its input) -- the whole priority list, first match wins.  usable(k): kernel k's own weights are packed (d.packed[k]:
// upload_layers), it is not switched off, and it takes the shape.  is_final: the network's last layer (Tanh epilogue) on an IH x IW
// logical input.  Also asked about LATER layers (acc_stats_ok, res_block_is_winograd), so it depends on nothing but its arguments.
ConvKernel select_conv(const ConvShape& s, const DevConvW& d, int precision, bool is_final, int IH, int IW, const Tuning& t)
{
    const auto usable = [&](ConvKernel k) {
        const ConvKernelInfo& r = conv_kernel(k);
        return (!r.pack || d.packed[k]) && !t.off[k] && (!r.eligible || r.eligible(s));
    };
    // only the generic kernel and the row-folded one (few output channels: kx taps folded into N) have the Tanh epilogue
    if (is_final) return usable(CK_FOLD) && conv_fold_launchable(s.cin_pitch, s.k, s.pad, s.ups, IH, IW) ? CK_FOLD : CK_GENERIC;
    // a transposed convolution (stride >= 2: upload() turns stride 1 into an ordinary convolution) by output phase on the physical input;
    // FAV_NO_TCONV: on the generic kernel, over the zero-stuffed input
    if (s.transposed) return usable(CK_TCONV) ? CK_TCONV : CK_GENERIC;
    // The first layer (9x9 on the 8-channel input pixel) by minimal filtering, ahead of its direct forms below: 2-D F(2x2,3x3) over its
    // nine 3x3 blocks, or 1-D F(2,3) along x on request (FAV_FIRST_1D).  FAV_NO_C8D takes both away together with the dense-K direct
    // form.  A layer that the c8 kernel does not take (more than 32 filters, FAV_NO_C8) has the 2-D form only, in groups of 32 filters
    const bool c8 = usable(CK_C8);
    if (!t.off[CK_C8D]) {
        if (c8 && usable(CK_FIRST1D)) return usable(CK_FIRST2D) && !t.first_1d ? CK_FIRST2D : CK_FIRST1D;
        if (!c8 && usable(CK_FIRST2D)) return CK_FIRST2D;
    }
    // 3x3 stride 2 (d64 / d128): the fragment-order kernel, ahead of the stride-2 halo kernel and the generic one that ran them before it
    if (usable(CK_S2W)) return CK_S2W;
    // 3x3 on a x2-upsampled input (fp32 only): four 2x2 convolutions on the physical pixels instead of a 3x3 on every logical one
    if (precision == 0 && usable(CK_UP2)) return CK_UP2;
    // unpadded 3x3 stride 1 (the residual blocks; fp32 only): Winograd F(4x4), or F(2x2) under FAV_WINO_F2 and where F(4x4) is not packed
    if (precision == 0 && !t.wino_f2 && usable(CK_WINO4)) return CK_WINO4;
    if (precision == 0 && usable(CK_WINO)) return CK_WINO;
    // the first layer's direct forms: dense K for its 7 (3) real input channels, else all 8
    if (c8) return usable(CK_C8D) ? CK_C8D : CK_C8;
    // the halo-resident implicit GEMMs take what is left of the 3x3 layers (bf16 fast mode, padded layers, FAV_NO_WINO / _UP2 / _S2W)
    if (usable(CK_HALO3)) return CK_HALO3;
    if (usable(CK_S2HALO)) return CK_S2HALO;
    return CK_GENERIC;
}

// kernel r's profile id for launch c (fav_internal.h, enum ConvKernel)
int profile_id(const ConvKernelInfo& r, const ConvLaunch& c)
{
    if (r.id_rule == ID_N_TILE) return c.COUTp % 128 == 0 ? 128 : (c.COUTp % 64 == 0 ? 64 : 32);
    return r.id + (r.id_rule == ID_FIXED ? 0 : c.COUTp) + (r.id_rule == ID_PLUS_N_JOIN && c.join_skip != nullptr ? 1 : 0);
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

}  // namespace

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
        dev_ptr<void> sp;
        const int rc = dev_alloc(sp, sz); if (rc) return rc;
        slab_cur = static_cast<char*>(sp.get()); slab_left = sz;
        slabs.push_back(std::move(sp));
    }
    DevBuf b; b.bytes = bytes; b.p = slab_cur;
    slab_cur += bytes; slab_left -= bytes;
    bufs.push_back(b); ++cursor;
    *out = static_cast<float*>(b.p);
    return FAV_OK;
}

int fav_net::timed_conv(const ConvLaunch& c, const Layer& L, ConvKernel kernel)
{
    const ConvKernelInfo& k = conv_kernel(kernel);
    const int conv_index = L.dev_index;
    if (c.pre.acc1 != nullptr && kernel != CK_WINO4) { set_error("internal: accumulator-form InstanceNorm in front of the %s kernel, which cannot take it", k.name); return FAV_EINVAL; }
    ConvLaunch cs = c;
    cs.reserve_cus = reserve_cus;
    cs.no_sk = shared_device ? 1 : 0;
    cs.sk_ws = sk_ws; cs.sk_flags = sk_flags; cs.sk_epoch = ++sk_epoch;      // launches of one net are stream-ordered
    cs.sk_err = sk_err_dev;
    cs.ks_ws = ks_ws; cs.ks_cnt = ks_cnt;
    if (sk_epoch == 0xffffffffu) sk_epoch = 0;
    // generic kernel while look-ahead masks are in flight: its stream-K hand-off assumes that all blocks are resident at once, and the
    // side queues' kernels land on any CU -- owners then wait for blocks that have not started (d128: 186 us against 115 us alone,
    // profiles/r02p_4arg_kernel_stats.csv).  Data-parallel grids do not wait for anybody.  The halo-resident 3x3 kernels (bf16 fast
    // mode, FAV_NO_WINO) hand tiles over the same way (ConvKernelInfo::hands_over)
    if (k.hands_over && reserve_cus > 0 && tuning().side_sk != 1 && !(tuning().side_sk == 2 && kernel == CK_S2HALO)) cs.no_sk = 1;
    char tag[96] = "";
    if (TraceRange::enabled()) snprintf(tag, sizeof tag, "fav:conv%d k%d s%d %d->%d %dx%d", conv_index, L.k, L.stride, L.cin, L.cout, c.OW, c.OH);
    TraceRange tr(tag);
    if (!profiling) return k.launch(cs, st);
    ProfRec r; r.conv = conv_index;
    // (no system-scope fence at the event: the default one flushes the caches around every timed kernel -- 6 us on either side of each
    // convolution in the rocprofv3 trace, 0.18 ms per 1280x720 frame)
    if (event_create(r.a, hipEventDisableSystemFence) || event_create(r.b, hipEventDisableSystemFence)) return FAV_EHIP;
    FAV_HIP(hipEventRecord(r.a.get(), st));
    int rc = k.launch(cs, st);
    FAV_HIP(hipEventRecord(r.b.get(), st));
    prof_pending.push_back(std::move(r));
    if ((int)prof_ms.size() <= conv_index) { prof_ms.resize(conv_index + 1, 0.0); prof_macs.resize(conv_index + 1, 0.0); prof_n.resize(conv_index + 1, 0); prof_tile.resize(conv_index + 1, 0); }
    prof_macs[conv_index] = (double)c.OH * c.OW * L.cout * L.cin * L.k * L.k;      // useful MACs only
    if (L.transposed) prof_macs[conv_index] /= (double)(L.stride * L.stride);       // (every output pixel meets k^2 / s^2 taps)
    prof_tile[conv_index] = profile_id(k, c);
    return rc;
}

// conv - InstanceNorm - ReLU - conv with both convolutions on the F(4x4) kernel (the first half of a residual branch,
// models_video.lua:10-39): the first convolution adds its units' statistics to the InstanceNorm's accumulators and the second forms
// scale / shift from them in its prologue -- no in_finalize launch between the two (round 5).  ls[li] = the first convolution
bool fav_net::acc_stats_ok(const std::vector<Layer>& ls, size_t li) const
{
    if (tuning().no_acc_stats) return false;
    if (li + 3 >= ls.size() || ls[li + 1].type != L_IN || ls[li + 2].type != L_RELU || ls[li + 3].type != L_CONV) return false;
    const DevConvW& d2 = convs[ls[li + 3].dev_index];
    return select_conv(with_input(d2.s, IN_NORM), d2, precision, false, 0, 0, tuning()) == CK_WINO4;      // (behind the InstanceNorm + ReLU: one pending stage)
}

// conv - InstanceNorm - ReLU - conv - InstanceNorm (models_video.lua:10-39) with both convolutions on the Winograd kernel
bool fav_net::res_block_is_winograd(const Layer& R) const
{
    const std::vector<Layer>& b = R.block;
    if (b.size() != 5 || b[0].type != L_CONV || b[1].type != L_IN || b[2].type != L_RELU || b[3].type != L_CONV || b[4].type != L_IN) return false;
    for (int k = 0; k < 2; ++k) {
        const DevConvW& d = convs[b[k ? 3 : 0].dev_index];
        const ConvKernel kernel = select_conv(with_input(d.s, IN_NORM), d, precision, false, 0, 0, tuning());
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
            const DevConvW& d = convs[L.dev_index];
            if (cur.C != d.s.cin_pitch) { set_error("internal: channel pitch mismatch (%d vs %d)", cur.C, d.s.cin_pitch); return FAV_EINVAL; }
            ConvLaunch c;
            c.in = cur.data; c.IH = cur.H(); c.IW = cur.W(); c.IWp = cur.P(); c.ups = cur.ups; c.CIN = d.s.cin_pitch; c.cin_real = L.cin;
            c.pre = cur.pre;
            c.wgt = d.wgt; c.bias = d.bias; c.COUT = L.cout; c.COUTp = d.s.coutp; c.KH = c.KW = L.k; c.stride = L.stride;
            c.pad = L.pad; c.Kpad = d.kpad;
            bool has_tanh = false; float mul = 1.f;
            const bool is_final = top && only_tail(ls, li + 1, has_tanh, mul) && has_tanh && L.cout == 3;
            if (L.transposed) {
                if (cur.ups != 0) { set_error("network: SpatialFullConvolution directly after an upsampling is unsupported"); return FAV_EUNSUPPORTED; }
                if (is_final) { set_error("network: a transposed convolution as the last layer is unsupported"); return FAV_EUNSUPPORTED; }
            }
            const ConvKernel kernel = select_conv(with_input(d.s, {cur.pre.stages, cur.ups}), d, precision, is_final, c.IH, c.IW, tuning());
            const ConvKernelInfo& k = conv_kernel(kernel);
            c.wpk = d.packed[kernel];
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
                int rc = timed_conv(c, L, kernel); if (rc) return rc;
                cur = nxt;
                return FAV_OK;        // Tanh / MulConstant / TotalVariation are folded into the epilogue
            }
            if (L.cout % 4 != 0) { set_error("network: %d output channels (must be a multiple of 4 except for the last layer)", L.cout); return FAV_EUNSUPPORTED; }
            const bool pitched_out = lazy.active && L.dev_index == lazy.conv_index;
            int rc;
            if (pitched_out) {
                // the output of a block whose join stays pending: pixel (i, j) at the linear index of the skip's pixel (i + shave, j + shave)
                if (c.OH != lazy.rows - 2 * lazy.shave || c.OW > lazy.pitch - 2 * lazy.shave) { set_error("internal: pending residual join of mismatching shapes"); return FAV_EINVAL; }
                float* base = nullptr;
                rc = alloc((size_t)lazy.rows * lazy.pitch * L.cout * sizeof(float), &base); if (rc) return rc;
                nxt.data = base + ((size_t)lazy.shave * lazy.pitch + lazy.shave) * L.cout; nxt.pitch = lazy.pitch; c.OWp = lazy.pitch;
            } else { rc = alloc((size_t)c.OH * c.OW * L.cout * sizeof(float), &nxt.data); if (rc) return rc; }
            const bool want_stats = li + 1 < ls.size() && ls[li + 1].type == L_IN;
            if (kernel == CK_HALO3 && precision == 1) c.wgt16 = d.wgt16;
            nxt.mblocks = k.tiles(c); nxt.ppitch = d.s.coutp;
            const bool acc = kernel == CK_WINO4 && want_stats && !pitched_out && cur.join_skip == nullptr &&
                             (acc_stats_ok(ls, li) || (branch_tail_acc_ok && !top && li + 2 == ls.size() && !tuning().no_acc_stats && precision == 0));
            if (acc) {
                DevIN& din = ins[ls[li + 1].dev_index];        // the InstanceNorm that follows
                nxt.acc = din.acc + (size_t)acc_parity * stat_acc_words(L.cout); nxt.acc_other = din.acc + (size_t)(acc_parity ^ 1) * stat_acc_words(L.cout);
                c.stat_acc = nxt.acc;
            }
            if (want_stats && !acc) { rc = alloc((size_t)nxt.mblocks * d.s.coutp * 2 * sizeof(float), &nxt.partials); if (rc) return rc; }
            if (want_stats && !acc && k.counts) { float* cp = nullptr; rc = alloc((size_t)nxt.mblocks * sizeof(int), &cp); if (rc) return rc; nxt.counts = reinterpret_cast<int*>(cp); }
            c.out = nxt.data; c.partials = nxt.partials;
            if (cur.join_skip != nullptr || pitched_out) {
                if (kernel != CK_WINO && kernel != CK_WINO4) { set_error("internal: a pending residual join next to a convolution that is not the Winograd kernel's"); return FAV_EINVAL; }
                c.join_skip = cur.join_skip; c.join_out = cur.join_out;
            }
            c.counts = k.counts ? (nxt.counts ? nxt.counts : reinterpret_cast<int*>(zeros)) : nullptr;
            rc = timed_conv(c, L, kernel); if (rc) return rc;
            cur = nxt;
            break;
        }
        case L_IN: {
            const DevIN& d = ins[L.dev_index];
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
            const DevIN& d = ins[L.dev_index];
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
            const bool lazy_out = !tuning().no_lazy_join && (tuning().wino_f2 || tuning().lazy_join) && precision == 0 &&
                                  li + 1 < ls.size() && ls[li + 1].type == L_RES && skip.pre.stages == 0 && skip.ups == 0 &&
                                  res_block_is_winograd(L) && res_block_is_winograd(ls[li + 1]);
            if (lazy_out) { lazy.active = true; lazy.pitch = skip.P(); lazy.rows = skip.Hp; lazy.shave = L.shave; lazy.conv_index = L.block[3].dev_index; }      // (the block's last convolution)
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
    if (sk_err_host && *static_cast<volatile unsigned*>(sk_err_host.get())) {      // reported by an earlier launch of this net
        *sk_err_host = 0;
        shared_device = true;
        set_error("a stream-K hand-off between convolution blocks timed out in an earlier launch of this network: its result was "
                  "wrong (two networks running concurrently on one device? see the concurrency note in fav.h)");
        return FAV_EHIP;
    }
    if (H != curH || W != curW) {
        if (!bufs.empty()) {
            FAV_HIP(hipDeviceSynchronize());
            slabs.clear(); slab_cur = nullptr; slab_left = 0;      // (frees them)
            bufs.clear();
        }
        curH = H; curW = W;
    }
    st = stream; cursor = 0;
    // InstanceNorm accumulators (Affine::acc1): a forward adds to one half and its consumers zero the other for the next one.  The halves
    // alternate over the forwards that USE them (fp32 mode; which layers do depends on the network and the process-wide switches only), so a
    // half is zero whenever it is added to -- unless a forward stopped between a producer and its consumer: then everything is zeroed here
    if (acc_dirty) {
        for (DevIN& i : ins) if (i.acc) FAV_HIP(hipMemsetAsync(i.acc, 0, i.acc_bytes, stream));
        acc_dirty = false;
    }
    if (precision == 0 && !tuning().no_acc_stats && !tuning().off[CK_WINO4]) acc_parity ^= 1;
    Act cur;
    cur.data = const_cast<float*>(in8); cur.Hp = H + 2 * pad; cur.Wp = W + 2 * pad; cur.C = 8;
    const int rc = run(exec, cur, true, out_planar, out_raw);
    if (rc) acc_dirty = true;
    return rc;
}

// ================================================================================================
// C ABI: network
// ================================================================================================
extern "C" int fav_net_create(const char* t7_path_host, int device, fav_net** out)
{
    FAV_REQUIRE(t7_path_host && out, "fav_net_create: null argument");
    int rc = ensure_device(); if (rc) return rc;
    FAV_ABI_TRY
    std::unique_ptr<fav_net> net(new fav_net());
    net->device = device;
    rc = t7_parse_model(t7_path_host, net->layers);
    if (!rc) rc = net->upload();
    if (!rc) *out = net.release();
    return rc;
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
    if (!rc) rc = net->upload();
    if (!rc) *out = net.release();
    return rc;
    FAV_ABI_CATCH("fav_net_create_from_blob")
}

extern "C" void fav_net_destroy(fav_net* net) { delete net; }

extern "C" int fav_net_check(fav_net* net)
{
    FAV_REQUIRE(net, "fav_net_check: null net");
    if (net->sk_err_host && *static_cast<volatile unsigned*>(net->sk_err_host.get())) {
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
        FAV_HIP(hipEventSynchronize(r.b.get()));
        float ms = 0.f;
        FAV_HIP(hipEventElapsedTime(&ms, r.a.get(), r.b.get()));
        net->prof_ms[r.conv] += ms; net->prof_n[r.conv] += 1;
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
        net->stage.reset(); net->stage_bytes = 0;
        int rc = dev_alloc(net->stage, bytes / sizeof(float)); if (rc) return rc;
        net->stage_bytes = bytes;
    }
    float* in8 = net->stage.get();
    int rc = launch_nchw_to_nhwc_pad(in7, net->in_channels, H, W, net->pad, 8, in8, st); if (rc) return rc;
    return net->forward_padded(in8, H, W, nullptr, out3, st);
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
