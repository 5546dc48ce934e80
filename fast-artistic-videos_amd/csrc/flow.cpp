// flow.cpp -- the coarse-to-fine optical-flow estimator behind fav_flow_rgb8 (kernels in kernels_flow.hip; the algorithm is stated in
// DESIGN.md, "fav_flow", and restated in numpy by tests/util/flow_model.py, for smooth_eps > 0 by tests/util/flow_robust_model.py and for the
// gradient-constancy data term by tests/util/flow_grad_model.py, for the matching prior by tests/util/flow_match_model.py, for the median
// filter between warps by tests/util/flow_median_model.py):
// option defaults, the layout of the caller's workspace and the sequence of launches.  Nothing here allocates or synchronises.
#include <cmath>

#include "fav_internal.h"

using namespace fav;

namespace {

constexpr int MAX_LEVELS = 6, MIN_SIDE = 16;
constexpr int DEFAULT_WARPS = 3, DEFAULT_ITERS = 30, DEFAULT_SWEEPS_PER_LAUNCH = 6;
constexpr float DEFAULT_ALPHA = 15.f, DEFAULT_ALPHA_ROBUST = 5.f;      // (robust: with smooth_eps > 0)
constexpr float DEFAULT_ALPHA_GRAD = 8.f, DEFAULT_ALPHA_GRAD_ROBUST = 8.f;      // with the gradient-constancy data term (measured)
constexpr float MIN_EPS = 1e-6f, MAX_EPS = 1e6f;                      // eps^2 and 1 / eps stay normal fp32 numbers
constexpr int MATCH_LEVEL = 1, DEFAULT_MATCH_RADIUS = 16;             // the matching prior ("Matching prior": measured)
constexpr float DEFAULT_MATCH_BETA = 225.f, MAX_MATCH_BETA = 1e6f, MATCH_TAU = 1.f, MATCH_TAU_LEVEL0 = 2.f;

// The workspace of a call on `images` images and `flows` flows (fav_flow_rgb8: 2 and 1; fav_flow_pairs_rgb8: 2 n and 2 n).  The planes
// of one kind at one level lie one behind the other, `stride` bytes apart (a multiple of 256).
struct FlowPlan {
    int levels = 0, warps = 0, iters = 0, K = 0, images = 0, flows = 0;
    FlowVariant v = {0.f, 0.f, false, nullptr};                              // eps > 0: edge-preserving smoothness (wgt: set by run_plan)
    int w[MAX_LEVELS], h[MAX_LEVELS];
    size_t pyr[MAX_LEVELS], pyr_stride[MAX_LEVELS];                          // byte offsets into the workspace: `images` grey planes
    size_t flow0[MAX_LEVELS], flow1[MAX_LEVELS], flow_stride[MAX_LEVELS];    // the two flow buffers of a level, `flows` planes each (level 0:
                                                                             // flow1 only, the other ones are the caller's)
    size_t coef = 0, coef_stride = 0, wgt = 0, wgt_stride = 0, bytes = 0;    // wgt: the edge weights (eps > 0 only)
    // the matching prior (beta > 0 only): `matches` match fields of level 1 (one per flow and direction: 2 for a single flow, else the
    // flows themselves, whose opposites are in the batch), and per flow the prior planes of the levels >= 1 (level 0 reads level 1's)
    float beta = 0.f;
    int radius = 0, matches = 0;
    size_t match = 0, match_stride = 0, prior[MAX_LEVELS] = {}, prior_stride[MAX_LEVELS] = {};
    int median = 0;      // 3 | 5: the window of the median filter behind every warp's sweeps; it owns no part of the workspace
};

// FAV_OK or FAV_EINVAL (message set)
int make_plan(int W, int H, const fav_flow_opts_ex3* ex3, int images, int flows, FlowPlan& p)
{
    static const fav_flow_opts_ex3 none = flow_opts_no_median(nullptr);
    if (!ex3) ex3 = &none;
    const fav_flow_opts_ex2* ex2 = &ex3->ex2;
    const fav_flow_opts_ex* ex = &ex2->ex;
    const fav_flow_opts* o = &ex->base;
    FAV_REQUIRE(ex3->median == 0 || ex3->median == 3 || ex3->median == 5, "fav_flow: median must be 0 (off), 3 or 5 (the side of the window), not %d", ex3->median);
    p.median = ex3->median;
    FAV_REQUIRE(std::isfinite(ex2->match_beta) && ex2->match_beta <= MAX_MATCH_BETA, "fav_flow: match_beta must be 0 (off), negative (default) or a number up to 1e6, not %g",
                (double)ex2->match_beta);
    FAV_REQUIRE(ex2->match_radius >= 0 && ex2->match_radius <= FLOW_MATCH_MAX_RADIUS, "fav_flow: match_radius must be 0 (default) .. %d, not %d", FLOW_MATCH_MAX_RADIUS,
                ex2->match_radius);
    p.beta = ex2->match_beta < 0.f ? DEFAULT_MATCH_BETA : ex2->match_beta;
    p.radius = ex2->match_radius ? ex2->match_radius : DEFAULT_MATCH_RADIUS;
    FAV_REQUIRE(ex->data_term == FAV_FLOW_DATA_BRIGHTNESS || ex->data_term == FAV_FLOW_DATA_GRADIENT,
                "fav_flow: data_term must be 0 (brightness constancy) or 1 (gradient constancy), not %d", ex->data_term);
    p.v.grad = ex->data_term == FAV_FLOW_DATA_GRADIENT;
    FAV_REQUIRE(W >= MIN_SIDE && H >= MIN_SIDE && (long long)W * H <= (1ll << 28), "fav_flow: frames must be at least %dx%d (and at most 2^28 pixels), not %dx%d", MIN_SIDE, MIN_SIDE, W, H);
    FAV_REQUIRE(o->levels >= 0 && o->levels <= MAX_LEVELS, "fav_flow: levels must be 0 (default) .. %d, not %d", MAX_LEVELS, o->levels);
    FAV_REQUIRE(o->warps >= 0 && o->warps <= 32, "fav_flow: warps must be 0 (default) .. 32, not %d", o->warps);
    FAV_REQUIRE(o->iters >= 0 && o->iters <= 1000, "fav_flow: iters must be 0 (default) .. 1000, not %d", o->iters);
    FAV_REQUIRE(std::isfinite(o->alpha) && o->alpha >= 0.f && o->alpha <= 1e6f, "fav_flow: alpha must be 0 (default) or a positive number up to 1e6, not %g", (double)o->alpha);
    FAV_REQUIRE(o->sweeps_per_launch >= 0 && o->sweeps_per_launch <= FLOW_MAX_SWEEPS_PER_LAUNCH, "fav_flow: sweeps_per_launch must be 0 (default) .. %d, not %d", FLOW_MAX_SWEEPS_PER_LAUNCH, o->sweeps_per_launch);
    FAV_REQUIRE(o->smooth_eps == 0.f || (std::isfinite(o->smooth_eps) && o->smooth_eps >= MIN_EPS && o->smooth_eps <= MAX_EPS),
                "fav_flow: smooth_eps must be 0 (off) or a number in 1e-6 .. 1e6, not %g", (double)o->smooth_eps);
    p.v.eps = o->smooth_eps;
    p.warps = o->warps ? o->warps : DEFAULT_WARPS;
    p.iters = o->iters ? o->iters : DEFAULT_ITERS;
    p.v.alpha = o->alpha != 0.f ? o->alpha
              : p.v.grad ? (p.v.eps > 0.f ? DEFAULT_ALPHA_GRAD_ROBUST : DEFAULT_ALPHA_GRAD) : (p.v.eps > 0.f ? DEFAULT_ALPHA_ROBUST : DEFAULT_ALPHA);
    p.K = o->sweeps_per_launch ? o->sweeps_per_launch : DEFAULT_SWEEPS_PER_LAUNCH;
    p.images = images; p.flows = flows;
    p.w[0] = W; p.h[0] = H; p.levels = 1;
    // a level is added while its smaller side is still >= 16, at most 6; an explicit count is taken as given
    while (o->levels ? p.levels < o->levels
                     : (p.levels < MAX_LEVELS && std::min((p.w[p.levels - 1] + 1) / 2, (p.h[p.levels - 1] + 1) / 2) >= MIN_SIDE)) {
        p.w[p.levels] = (p.w[p.levels - 1] + 1) / 2; p.h[p.levels] = (p.h[p.levels - 1] + 1) / 2;
        ++p.levels;
    }
    FAV_REQUIRE(p.beta == 0.f || p.levels > MATCH_LEVEL, "fav_flow: the matching prior (match_beta) needs a pyramid of at least two levels, %dx%d with levels %d has one", W, H, o->levels);
    size_t off = 0;
    auto round256 = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
    auto take = [&](size_t stride, int count) { const size_t at = off; off += stride * count; return at; };
    for (int l = 0; l < p.levels; ++l) {
        const size_t n = (size_t)p.w[l] * p.h[l];
        p.pyr_stride[l] = round256(n * 4); p.flow_stride[l] = round256(n * 8);
        p.pyr[l] = take(p.pyr_stride[l], images);
        p.flow0[l] = l ? take(p.flow_stride[l], flows) : 0; p.flow1[l] = take(p.flow_stride[l], flows);
    }
    p.coef_stride = round256((size_t)W * H * (p.v.grad || p.beta > 0.f ? 20 : 16));
    p.coef = take(p.coef_stride, flows);
    p.wgt_stride = round256((size_t)W * H * 16);
    if (p.v.eps > 0.f) p.wgt = take(p.wgt_stride, flows);
    if (p.beta > 0.f) {
        p.matches = flows == 1 ? 2 : flows;
        p.match_stride = round256((size_t)p.w[MATCH_LEVEL] * p.h[MATCH_LEVEL] * 4);
        p.match = take(p.match_stride, p.matches);
        for (int l = MATCH_LEVEL; l < p.levels; ++l) {
            p.prior_stride[l] = round256((size_t)p.w[l] * p.h[l] * 12);
            p.prior[l] = take(p.prior_stride[l], flows);
        }
    }
    p.bytes = off;
    return FAV_OK;
}

// The launches of a call.  img: the plan's images; flow j is the one with A = image a_of[j], B = image b_of[j] and ends in out.p[j].
int run_plan(const FlowPlan& p, const FlowPtrs& img, const int* a_of, const int* b_of, const FlowPtrs& out, char* ws, hipStream_t st)
{
    int rc;
    // grey + pyramids: every image once
    FlowPtrs finer(ws + p.pyr[0], p.pyr_stride[0], p.images);
    rc = launch_flow_grey(img, finer, p.images, p.w[0], p.h[0], st); if (rc) return rc;
    for (int l = 1; l < p.levels; ++l) {
        const FlowPtrs level(ws + p.pyr[l], p.pyr_stride[l], p.images);
        rc = launch_flow_down(finer, p.w[l - 1], p.h[l - 1], level, p.images, st); if (rc) return rc;
        finer = level;
    }
    // coarse to fine.  Every warp ends ceil(iters / K) buffer swaps later, and one more with the median filter (it goes from the buffer the
    // sweeps ended in into the other one): level 0 starts in the buffers that leave the results in `out`
    const int swaps = p.warps * ((p.iters + p.K - 1) / p.K + (p.median ? 1 : 0));
    const FlowPtrs coef(ws + p.coef, p.coef_stride, p.flows);
    const FlowPtrs wgt_planes(ws + p.wgt, p.wgt_stride, p.flows);
    FlowVariant v = p.v;
    if (v.eps > 0.f) v.wgt = &wgt_planes;
    // the matching prior: one match launch over every flow and its opposite (a single flow: the two directions of its pair; a batch: its
    // own flows, backward k and forward k being each other's opposite), the check, and the coarser levels' planes
    if (p.beta > 0.f) {
        const int l = MATCH_LEVEL, half = p.flows / 2;
        FlowPtrs mA, mB, own, opp;
        const FlowPtrs fields(ws + p.match, p.match_stride, p.matches);
        for (int i = 0; i < p.matches; ++i) {
            const int j = p.flows == 1 ? 0 : i;
            const bool swap = p.flows == 1 && i == 1;
            mA.p[i] = ws + p.pyr[l] + (swap ? b_of[j] : a_of[j]) * p.pyr_stride[l];
            mB.p[i] = ws + p.pyr[l] + (swap ? a_of[j] : b_of[j]) * p.pyr_stride[l];
        }
        for (int j = 0; j < p.flows; ++j) { own.p[j] = fields.p[j]; opp.p[j] = fields.p[p.flows == 1 ? 1 : (j + half) % p.flows]; }
        rc = launch_flow_match(mA, mB, fields, p.matches, p.w[l], p.h[l], p.radius, st); if (rc) return rc;
        FlowPtrs finer_prior(ws + p.prior[l], p.prior_stride[l], p.flows);
        rc = launch_flow_match_check(own, opp, finer_prior, p.flows, p.w[l], p.h[l], st); if (rc) return rc;
        for (int c = l + 1; c < p.levels; ++c) {
            const FlowPtrs level(ws + p.prior[c], p.prior_stride[c], p.flows);
            rc = launch_flow_prior_down(finer_prior, p.w[c - 1], p.h[c - 1], level, p.flows, st); if (rc) return rc;
            finer_prior = level;
        }
    }
    FlowPrior prior;
    FlowPtrs coarser;
    for (int l = p.levels - 1; l >= 0; --l) {
        FlowPtrs cur = l ? FlowPtrs(ws + p.flow0[l], p.flow_stride[l], p.flows) : out;
        FlowPtrs other(ws + p.flow1[l], p.flow_stride[l], p.flows);
        if (l == 0 && (swaps & 1)) std::swap(cur, other);
        const bool cur_in_workspace = l != 0 || (swaps & 1);      // then its planes are one range from cur.p[0], flow_stride apart
        const int w = p.w[l], h = p.h[l];
        FlowPtrs A, B;
        for (int j = 0; j < p.flows; ++j) {
            A.p[j] = ws + p.pyr[l] + a_of[j] * p.pyr_stride[l];
            B.p[j] = ws + p.pyr[l] + b_of[j] * p.pyr_stride[l];
        }
        if (l == p.levels - 1) {                   // the coarsest level starts from zero (in the workspace: padding included)
            if (cur_in_workspace) FAV_HIP(hipMemsetAsync(cur.p[0], 0, p.flow_stride[l] * p.flows, st));
            else for (int j = 0; j < p.flows; ++j) FAV_HIP(hipMemsetAsync(cur.p[j], 0, (size_t)w * h * 8, st));
        } else { rc = launch_flow_up(coarser, p.w[l + 1], p.h[l + 1], cur, p.flows, w, h, st); if (rc) return rc; }
        if (p.beta > 0.f) {                        // level 0 reads level 1's planes at (x >> 1, y >> 1)
            const int pl = std::max(l, MATCH_LEVEL);
            prior = {FlowPtrs(ws + p.prior[pl], p.prior_stride[pl], p.flows), p.w[pl], p.h[pl], pl - l, (float)w / (float)p.w[pl], (float)h / (float)p.h[pl], p.beta,
                     l ? MATCH_TAU : MATCH_TAU_LEVEL0};
            v.prior = &prior;
        }
        for (int k = 0; k < p.warps; ++k) {
            rc = launch_flow_coef(A, B, cur, coef, v, p.flows, w, h, st); if (rc) return rc;
            rc = launch_flow_sweeps(&cur, &other, coef, v, p.flows, p.iters, p.K, w, h, st); if (rc) return rc;
            if (p.median) {
                rc = launch_flow_median(cur, other, p.flows, w, h, p.median, st); if (rc) return rc;
                std::swap(cur, other);
            }
        }
        coarser = cur;
    }
    return FAV_OK;
}

bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

extern "C" size_t fav_flow_workspace_bytes_ex(int W, int H, const fav_flow_opts_ex* opts_host)
{
    const fav_flow_opts_ex2 ex2 = flow_opts_no_match(opts_host);
    return fav_flow_workspace_bytes_ex2(W, H, &ex2);
}

extern "C" size_t fav_flow_workspace_bytes_ex2(int W, int H, const fav_flow_opts_ex2* opts_host)
{
    const fav_flow_opts_ex3 ex3 = flow_opts_no_median(opts_host);
    return fav_flow_workspace_bytes_ex3(W, H, &ex3);
}

extern "C" size_t fav_flow_workspace_bytes_ex3(int W, int H, const fav_flow_opts_ex3* opts_host)
{
    FlowPlan p;
    return make_plan(W, H, opts_host, 2, 1, p) ? 0 : p.bytes;
}

extern "C" size_t fav_flow_workspace_bytes(int W, int H, const fav_flow_opts* opts_host)
{
    const fav_flow_opts_ex ex = flow_opts_brightness(opts_host);
    return fav_flow_workspace_bytes_ex(W, H, &ex);
}

extern "C" int fav_flow_rgb8(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts* opts_host, float* flow_out,
                             void* workspace, size_t workspace_bytes, fav_hipstream_t stream)
{
    const fav_flow_opts_ex ex = flow_opts_brightness(opts_host);
    return fav_flow_rgb8_ex(a_rgb_hwc, b_rgb_hwc, W, H, &ex, flow_out, workspace, workspace_bytes, stream);
}

extern "C" int fav_flow_rgb8_ex(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts_ex* opts_host, float* flow_out,
                                void* workspace, size_t workspace_bytes, fav_hipstream_t stream)
{
    const fav_flow_opts_ex2 ex2 = flow_opts_no_match(opts_host);
    return fav_flow_rgb8_ex2(a_rgb_hwc, b_rgb_hwc, W, H, &ex2, flow_out, workspace, workspace_bytes, stream);
}

extern "C" int fav_flow_rgb8_ex2(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts_ex2* opts_host, float* flow_out,
                                 void* workspace, size_t workspace_bytes, fav_hipstream_t stream)
{
    const fav_flow_opts_ex3 ex3 = flow_opts_no_median(opts_host);
    return fav_flow_rgb8_ex3(a_rgb_hwc, b_rgb_hwc, W, H, &ex3, flow_out, workspace, workspace_bytes, stream);
}

extern "C" int fav_flow_rgb8_ex3(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts_ex3* opts_host, float* flow_out,
                                 void* workspace, size_t workspace_bytes, fav_hipstream_t stream)
{
    FlowPlan p;
    int rc = make_plan(W, H, opts_host, 2, 1, p); if (rc) return rc;
    FAV_REQUIRE(a_rgb_hwc && b_rgb_hwc && flow_out && workspace, "fav_flow_rgb8: null pointer");
    FAV_REQUIRE(workspace_bytes >= p.bytes, "fav_flow_rgb8: the workspace holds %zu bytes, fav_flow_workspace_bytes asks for %zu", workspace_bytes, p.bytes);
    FAV_REQUIRE(aligned(workspace, 16) && aligned(flow_out, 8), "fav_flow_rgb8: the workspace must be 16-byte aligned, flow_out 8-byte aligned");
    rc = ensure_device(); if (rc) return rc;
    FlowPtrs img; img.p[0] = const_cast<uint8_t*>(a_rgb_hwc); img.p[1] = const_cast<uint8_t*>(b_rgb_hwc);
    const int a_of = 0, b_of = 1;
    return run_plan(p, img, &a_of, &b_of, FlowPtrs(flow_out), static_cast<char*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" size_t fav_flow_pairs_workspace_bytes(int W, int H, int n_pairs, const fav_flow_opts* opts_host)
{
    const fav_flow_opts_ex ex = flow_opts_brightness(opts_host);
    return fav_flow_pairs_workspace_bytes_ex(W, H, n_pairs, &ex);
}

extern "C" int fav_flow_pairs_rgb8(const uint8_t* const* prev_rgb_hwc, const uint8_t* const* cur_rgb_hwc, int n_pairs, int W, int H,
                                   const fav_flow_opts* opts_host, float* const* backward_flo, float* const* forward_flo, void* workspace,
                                   size_t workspace_bytes, fav_hipstream_t stream)
{
    const fav_flow_opts_ex ex = flow_opts_brightness(opts_host);
    return fav_flow_pairs_rgb8_ex(prev_rgb_hwc, cur_rgb_hwc, n_pairs, W, H, &ex, backward_flo, forward_flo, workspace, workspace_bytes, stream);
}

extern "C" size_t fav_flow_pairs_workspace_bytes_ex(int W, int H, int n_pairs, const fav_flow_opts_ex* opts_host)
{
    const fav_flow_opts_ex2 ex2 = flow_opts_no_match(opts_host);
    return fav_flow_pairs_workspace_bytes_ex2(W, H, n_pairs, &ex2);
}

extern "C" size_t fav_flow_pairs_workspace_bytes_ex2(int W, int H, int n_pairs, const fav_flow_opts_ex2* opts_host)
{
    const fav_flow_opts_ex3 ex3 = flow_opts_no_median(opts_host);
    return fav_flow_pairs_workspace_bytes_ex3(W, H, n_pairs, &ex3);
}

extern "C" size_t fav_flow_pairs_workspace_bytes_ex3(int W, int H, int n_pairs, const fav_flow_opts_ex3* opts_host)
{
    FlowPlan p;
    if (n_pairs < 1 || n_pairs > FAV_FLOW_MAX_PAIRS) { set_error("fav_flow_pairs: n_pairs must be 1 .. %d, not %d", FAV_FLOW_MAX_PAIRS, n_pairs); return 0; }
    return make_plan(W, H, opts_host, 2 * n_pairs, 2 * n_pairs, p) ? 0 : p.bytes;
}

extern "C" int fav_flow_pairs_rgb8_ex(const uint8_t* const* prev_rgb_hwc, const uint8_t* const* cur_rgb_hwc, int n_pairs, int W, int H,
                                      const fav_flow_opts_ex* opts_host, float* const* backward_flo, float* const* forward_flo, void* workspace,
                                      size_t workspace_bytes, fav_hipstream_t stream)
{
    const fav_flow_opts_ex2 ex2 = flow_opts_no_match(opts_host);
    return fav_flow_pairs_rgb8_ex2(prev_rgb_hwc, cur_rgb_hwc, n_pairs, W, H, &ex2, backward_flo, forward_flo, workspace, workspace_bytes, stream);
}

extern "C" int fav_flow_pairs_rgb8_ex2(const uint8_t* const* prev_rgb_hwc, const uint8_t* const* cur_rgb_hwc, int n_pairs, int W, int H,
                                       const fav_flow_opts_ex2* opts_host, float* const* backward_flo, float* const* forward_flo, void* workspace,
                                       size_t workspace_bytes, fav_hipstream_t stream)
{
    const fav_flow_opts_ex3 ex3 = flow_opts_no_median(opts_host);
    return fav_flow_pairs_rgb8_ex3(prev_rgb_hwc, cur_rgb_hwc, n_pairs, W, H, &ex3, backward_flo, forward_flo, workspace, workspace_bytes, stream);
}

extern "C" int fav_flow_pairs_rgb8_ex3(const uint8_t* const* prev_rgb_hwc, const uint8_t* const* cur_rgb_hwc, int n_pairs, int W, int H,
                                       const fav_flow_opts_ex3* opts_host, float* const* backward_flo, float* const* forward_flo, void* workspace,
                                       size_t workspace_bytes, fav_hipstream_t stream)
{
    FAV_REQUIRE(n_pairs >= 1 && n_pairs <= FAV_FLOW_MAX_PAIRS, "fav_flow_pairs_rgb8: n_pairs must be 1 .. %d, not %d", FAV_FLOW_MAX_PAIRS, n_pairs);
    const int n = n_pairs;
    FlowPlan p;
    int rc = make_plan(W, H, opts_host, 2 * n, 2 * n, p); if (rc) return rc;
    FAV_REQUIRE(prev_rgb_hwc && cur_rgb_hwc && backward_flo && forward_flo && workspace, "fav_flow_pairs_rgb8: null pointer");
    // images: prev 0 .. n-1, cur 0 .. n-1;  flows: backward 0 .. n-1 (A = cur k, B = prev k), forward 0 .. n-1 (A = prev k, B = cur k)
    FlowPtrs img, out;
    int a_of[FLOW_MAX_ITEMS], b_of[FLOW_MAX_ITEMS];
    for (int k = 0; k < n; ++k) {
        FAV_REQUIRE(prev_rgb_hwc[k] && cur_rgb_hwc[k] && backward_flo[k] && forward_flo[k], "fav_flow_pairs_rgb8: null pointer in slot %d", k);
        FAV_REQUIRE(aligned(backward_flo[k], 8) && aligned(forward_flo[k], 8), "fav_flow_pairs_rgb8: the flows of slot %d must be 8-byte aligned", k);
        img.p[k] = const_cast<uint8_t*>(prev_rgb_hwc[k]); img.p[n + k] = const_cast<uint8_t*>(cur_rgb_hwc[k]);
        out.p[k] = backward_flo[k]; out.p[n + k] = forward_flo[k];
        a_of[k] = n + k; b_of[k] = k;
        a_of[n + k] = k; b_of[n + k] = n + k;
    }
    for (int i = 0; i < 2 * n; ++i)
        for (int j = 0; j < i; ++j)
            FAV_REQUIRE(out.p[i] != out.p[j], "fav_flow_pairs_rgb8: two outputs are one buffer (%s_flo[%d] and %s_flo[%d])",
                        j < n ? "backward" : "forward", j % n, i < n ? "backward" : "forward", i % n);
    FAV_REQUIRE(workspace_bytes >= p.bytes, "fav_flow_pairs_rgb8: the workspace holds %zu bytes, fav_flow_pairs_workspace_bytes asks for %zu", workspace_bytes, p.bytes);
    FAV_REQUIRE(aligned(workspace, 16), "fav_flow_pairs_rgb8: the workspace must be 16-byte aligned");
    rc = ensure_device(); if (rc) return rc;
    return run_plan(p, img, a_of, b_of, out, static_cast<char*>(workspace), static_cast<hipStream_t>(stream));
}

// ---- the stages on their own (tests: each is held to tests/util/flow_model.py)
extern "C" int fav_flow_grey_f32(const uint8_t* rgb_hwc, float* grey, int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_hwc && grey && W > 0 && H > 0, "fav_flow_grey_f32: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_grey(FlowPtrs(rgb_hwc), FlowPtrs(grey), 1, W, H, static_cast<hipStream_t>(stream));
}

extern "C" int fav_flow_down_f32(const float* src, float* dst, int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(src && dst && W > 0 && H > 0, "fav_flow_down_f32: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_down(FlowPtrs(src), W, H, FlowPtrs(dst), 1, static_cast<hipStream_t>(stream));
}

extern "C" int fav_flow_up_f32(const float* coarse_flow, int Wc, int Hc, float* fine_flow, int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(coarse_flow && fine_flow && Wc > 0 && Hc > 0 && W > 0 && H > 0, "fav_flow_up_f32: bad argument");
    FAV_REQUIRE(aligned(coarse_flow, 8) && aligned(fine_flow, 8), "fav_flow_up_f32: flows must be 8-byte aligned");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_up(FlowPtrs(coarse_flow), Wc, Hc, FlowPtrs(fine_flow), 1, W, H, static_cast<hipStream_t>(stream));
}

namespace {

// the coefficient entries: `weights` == nullptr is the quadratic smoothness term (smooth_eps is not read); grad: the gradient-constancy
// term (coef: five planes [5][H][W], 4-byte aligned)
int coef_entry(const char* who, const float* a_grey, const float* b_grey, const float* flow0, float alpha, float smooth_eps, float* coef, float* weights,
               int W, int H, fav_hipstream_t stream, bool grad, const FlowPrior* prior = nullptr)
{
    FAV_REQUIRE(a_grey && b_grey && flow0 && coef && W > 0 && H > 0 && std::isfinite(alpha) && alpha > 0.f, "%s: bad argument", who);
    const bool data_grad = grad;
    if (prior) grad = true;      // below, `grad` only says that coef is the five planes
    FAV_REQUIRE(!weights || (std::isfinite(smooth_eps) && smooth_eps >= MIN_EPS && smooth_eps <= MAX_EPS), "%s: smooth_eps must be a number in 1e-6 .. 1e6, not %g", who, (double)smooth_eps);
    FAV_REQUIRE(aligned(flow0, 8) && aligned(coef, grad ? 4 : 16) && aligned(weights, 16) && coef != weights, "%s: flow0 must be 8-byte aligned, coef %s", who,
                grad ? "4-byte aligned, weights 16-byte aligned and distinct from coef" : weights ? "and weights 16-byte aligned and distinct" : "16-byte aligned");
    int rc = ensure_device(); if (rc) return rc;
    const FlowPtrs wgt(weights);
    return launch_flow_coef(FlowPtrs(a_grey), FlowPtrs(b_grey), FlowPtrs(flow0), FlowPtrs(coef), {alpha, weights ? smooth_eps : 0.f, data_grad, weights ? &wgt : nullptr, prior},
                            1, W, H, static_cast<hipStream_t>(stream));
}

// the sweep entries: `weights` == nullptr is the plain mean; grad: the tensor form (coef: five planes, 4-byte aligned)
int sweeps_entry(const char* who, const float* flow0, const float* coef, const float* weights, int iters, int sweeps_per_launch, float* flow_out,
                 float* scratch, int W, int H, fav_hipstream_t stream, bool grad)
{
    FAV_REQUIRE(flow0 && coef && flow_out && scratch && W > 0 && H > 0, "%s: bad argument", who);
    FAV_REQUIRE(iters >= 1 && sweeps_per_launch >= 0 && sweeps_per_launch <= FLOW_MAX_SWEEPS_PER_LAUNCH, "%s: iters must be >= 1, sweeps_per_launch 0 (default) .. %d", who, FLOW_MAX_SWEEPS_PER_LAUNCH);
    FAV_REQUIRE(aligned(flow0, 8) && aligned(flow_out, 8) && aligned(scratch, 8) && aligned(coef, grad ? 4 : 16) && aligned(weights, 16),
                "%s: flows must be 8-byte aligned, coef%s 16-byte aligned", who, grad ? " 4-byte aligned, weights" : weights ? " and weights" : "");
    int rc = ensure_device(); if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int K = sweeps_per_launch ? sweeps_per_launch : DEFAULT_SWEEPS_PER_LAUNCH;
    // flow0 is read only: the first launch goes from it into the buffer from which the remaining launches end in flow_out
    const int first = std::min(K, iters), rest_launches = (iters - first + K - 1) / K;
    FlowPtrs src(flow0), cur((rest_launches & 1) ? scratch : flow_out), other((rest_launches & 1) ? flow_out : scratch), first_dst = cur;
    const FlowPtrs cf(coef), wgt(weights);
    const FlowVariant v = {0.f, 0.f, grad, weights ? &wgt : nullptr};      // (the sweeps read neither alpha nor eps)
    rc = launch_flow_sweeps(&src, &first_dst, cf, v, 1, first, K, W, H, st); if (rc) return rc;
    if (iters > first) { rc = launch_flow_sweeps(&cur, &other, cf, v, 1, iters - first, K, W, H, st); if (rc) return rc; }
    return FAV_OK;
}

}  // namespace

extern "C" int fav_flow_coefficients_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float* coef, int W, int H,
                                         fav_hipstream_t stream)
{
    return coef_entry("fav_flow_coefficients_f32", a_grey, b_grey, flow0, alpha, 0.f, coef, nullptr, W, H, stream, false);
}

extern "C" int fav_flow_coefficients_robust_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float smooth_eps, float* coef,
                                                float* weights, int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(weights, "fav_flow_coefficients_robust_f32: bad argument");
    return coef_entry("fav_flow_coefficients_robust_f32", a_grey, b_grey, flow0, alpha, smooth_eps, coef, weights, W, H, stream, false);
}

extern "C" int fav_flow_coefficients_grad_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float smooth_eps, float* coef,
                                              float* weights, int W, int H, fav_hipstream_t stream)
{
    return coef_entry("fav_flow_coefficients_grad_f32", a_grey, b_grey, flow0, alpha, smooth_eps, coef, weights, W, H, stream, true);
}

extern "C" int fav_flow_sweeps_f32(const float* flow0, const float* coef, int iters, int sweeps_per_launch, float* flow_out, float* scratch,
                                   int W, int H, fav_hipstream_t stream)
{
    return sweeps_entry("fav_flow_sweeps_f32", flow0, coef, nullptr, iters, sweeps_per_launch, flow_out, scratch, W, H, stream, false);
}

extern "C" int fav_flow_sweeps_robust_f32(const float* flow0, const float* coef, const float* weights, int iters, int sweeps_per_launch, float* flow_out,
                                          float* scratch, int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(weights, "fav_flow_sweeps_robust_f32: bad argument");
    return sweeps_entry("fav_flow_sweeps_robust_f32", flow0, coef, weights, iters, sweeps_per_launch, flow_out, scratch, W, H, stream, false);
}

extern "C" int fav_flow_sweeps_grad_f32(const float* flow0, const float* coef, const float* weights, int iters, int sweeps_per_launch, float* flow_out,
                                        float* scratch, int W, int H, fav_hipstream_t stream)
{
    return sweeps_entry("fav_flow_sweeps_grad_f32", flow0, coef, weights, iters, sweeps_per_launch, flow_out, scratch, W, H, stream, true);
}

// ---- the median filter on its own (tests: equal to tests/util/flow_median_model.py value for value)
extern "C" int fav_flow_median_f32(const float* flow_in, float* flow_out, int W, int H, int size, fav_hipstream_t stream)
{
    FAV_REQUIRE(flow_in && flow_out && W > 0 && H > 0 && (long long)W * H <= (1ll << 28), "fav_flow_median_f32: bad argument");
    FAV_REQUIRE(size == 3 || size == 5, "fav_flow_median_f32: size must be 3 or 5 (the side of the window), not %d", size);
    FAV_REQUIRE(aligned(flow_in, 8) && aligned(flow_out, 8), "fav_flow_median_f32: flows must be 8-byte aligned");
    const uintptr_t in = reinterpret_cast<uintptr_t>(flow_in), out = reinterpret_cast<uintptr_t>(flow_out), bytes = (uintptr_t)W * H * 8;
    FAV_REQUIRE(in + bytes <= out || out + bytes <= in, "fav_flow_median_f32: flow_in and flow_out overlap (the filter is not in place)");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_median(FlowPtrs(flow_in), FlowPtrs(flow_out), 1, W, H, size, static_cast<hipStream_t>(stream));
}

// ---- the matching prior's stages (tests: held to tests/util/flow_match_model.py)
extern "C" int fav_flow_match_f32(const float* a_grey, const float* b_grey, int W, int H, int radius, int16_t* d_ab, int16_t* d_ba, fav_hipstream_t stream)
{
    FAV_REQUIRE(a_grey && b_grey && d_ab && d_ba && d_ab != d_ba && W > 0 && H > 0, "fav_flow_match_f32: bad argument");
    FAV_REQUIRE(radius >= 1 && radius <= FLOW_MATCH_MAX_RADIUS, "fav_flow_match_f32: radius must be 1 .. %d, not %d", FLOW_MATCH_MAX_RADIUS, radius);
    FAV_REQUIRE(aligned(d_ab, 4) && aligned(d_ba, 4), "fav_flow_match_f32: the match fields must be 4-byte aligned");
    int rc = ensure_device(); if (rc) return rc;
    FlowPtrs A, B, d;
    A.p[0] = const_cast<float*>(a_grey); B.p[0] = const_cast<float*>(b_grey); d.p[0] = d_ab;
    A.p[1] = const_cast<float*>(b_grey); B.p[1] = const_cast<float*>(a_grey); d.p[1] = d_ba;
    return launch_flow_match(A, B, d, 2, W, H, radius, static_cast<hipStream_t>(stream));
}

extern "C" int fav_flow_match_check(const int16_t* d_ab, const int16_t* d_ba, int W, int H, float* prior, fav_hipstream_t stream)
{
    FAV_REQUIRE(d_ab && d_ba && prior && W > 0 && H > 0, "fav_flow_match_check: bad argument");
    FAV_REQUIRE(aligned(d_ab, 4) && aligned(d_ba, 4) && aligned(prior, 4), "fav_flow_match_check: the match fields and the prior must be 4-byte aligned");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_match_check(FlowPtrs(d_ab), FlowPtrs(d_ba), FlowPtrs(prior), 1, W, H, static_cast<hipStream_t>(stream));
}

extern "C" int fav_flow_coefficients_prior_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float smooth_eps, int data_term,
                                               const float* prior, int Wp, int Hp, float beta, float tau, float* coef, float* weights, int W, int H,
                                               fav_hipstream_t stream)
{
    const char* who = "fav_flow_coefficients_prior_f32";
    FAV_REQUIRE(data_term == FAV_FLOW_DATA_BRIGHTNESS || data_term == FAV_FLOW_DATA_GRADIENT, "%s: data_term must be 0 or 1, not %d", who, data_term);
    FAV_REQUIRE(prior && aligned(prior, 4) && W > 0 && H > 0, "%s: bad argument", who);
    FAV_REQUIRE(std::isfinite(beta) && beta > 0.f && beta <= MAX_MATCH_BETA, "%s: beta must be a positive number up to 1e6, not %g", who, (double)beta);
    FAV_REQUIRE(std::isfinite(tau) && tau >= 0.f, "%s: tau must be a number >= 0, not %g", who, (double)tau);
    const bool same = Wp == W && Hp == H, parent = Wp == (W + 1) / 2 && Hp == (H + 1) / 2;
    FAV_REQUIRE(same || parent, "%s: the prior must have the level's size %dx%d or the next coarser level's, not %dx%d", who, W, H, Wp, Hp);
    const FlowPrior pr = {FlowPtrs(prior), Wp, Hp, same ? 0 : 1, (float)W / (float)Wp, (float)H / (float)Hp, beta, tau};
    return coef_entry(who, a_grey, b_grey, flow0, alpha, smooth_eps, coef, weights, W, H, stream, data_term == FAV_FLOW_DATA_GRADIENT, &pr);
}
