// flow.cpp -- the coarse-to-fine optical-flow estimator behind fav_flow_rgb8 (kernels in kernels_flow.hip; the algorithm is stated in
// DESIGN.md, "fav_flow", and restated in numpy by tests/util/flow_model.py): option defaults, the layout of the caller's workspace and
// the sequence of launches.  Nothing here allocates or synchronises.
#include <cmath>

#include "fav_internal.h"

using namespace fav;

namespace {

constexpr int MAX_LEVELS = 6, MIN_SIDE = 16;
constexpr int DEFAULT_WARPS = 3, DEFAULT_ITERS = 30, DEFAULT_SWEEPS_PER_LAUNCH = 6;
constexpr float DEFAULT_ALPHA = 15.f;

struct FlowPlan {
    int levels = 0, warps = 0, iters = 0, K = 0;
    float alpha = 0.f;
    int w[MAX_LEVELS], h[MAX_LEVELS];
    size_t pyr_a[MAX_LEVELS], pyr_b[MAX_LEVELS];      // byte offsets into the workspace
    size_t flow0[MAX_LEVELS], flow1[MAX_LEVELS];      // the two flow buffers of a level (level 0: flow1 only, the other one is flow_out)
    size_t coef = 0, bytes = 0;
};

// FAV_OK or FAV_EINVAL (message set)
int make_plan(int W, int H, const fav_flow_opts* o, FlowPlan& p)
{
    static const fav_flow_opts none = {0, 0, 0, 0.f, 0};
    if (!o) o = &none;
    FAV_REQUIRE(W >= MIN_SIDE && H >= MIN_SIDE && (long long)W * H <= (1ll << 28), "fav_flow: frames must be at least %dx%d (and at most 2^28 pixels), not %dx%d", MIN_SIDE, MIN_SIDE, W, H);
    FAV_REQUIRE(o->levels >= 0 && o->levels <= MAX_LEVELS, "fav_flow: levels must be 0 (default) .. %d, not %d", MAX_LEVELS, o->levels);
    FAV_REQUIRE(o->warps >= 0 && o->warps <= 32, "fav_flow: warps must be 0 (default) .. 32, not %d", o->warps);
    FAV_REQUIRE(o->iters >= 0 && o->iters <= 1000, "fav_flow: iters must be 0 (default) .. 1000, not %d", o->iters);
    FAV_REQUIRE(std::isfinite(o->alpha) && o->alpha >= 0.f && o->alpha <= 1e6f, "fav_flow: alpha must be 0 (default) or a positive number up to 1e6, not %g", (double)o->alpha);
    FAV_REQUIRE(o->sweeps_per_launch >= 0 && o->sweeps_per_launch <= FLOW_MAX_SWEEPS_PER_LAUNCH, "fav_flow: sweeps_per_launch must be 0 (default) .. %d, not %d", FLOW_MAX_SWEEPS_PER_LAUNCH, o->sweeps_per_launch);
    p.warps = o->warps ? o->warps : DEFAULT_WARPS;
    p.iters = o->iters ? o->iters : DEFAULT_ITERS;
    p.alpha = o->alpha != 0.f ? o->alpha : DEFAULT_ALPHA;
    p.K = o->sweeps_per_launch ? o->sweeps_per_launch : DEFAULT_SWEEPS_PER_LAUNCH;
    p.w[0] = W; p.h[0] = H; p.levels = 1;
    // a level is added while its smaller side is still >= 16, at most 6; an explicit count is taken as given
    while (o->levels ? p.levels < o->levels
                     : (p.levels < MAX_LEVELS && std::min((p.w[p.levels - 1] + 1) / 2, (p.h[p.levels - 1] + 1) / 2) >= MIN_SIDE)) {
        p.w[p.levels] = (p.w[p.levels - 1] + 1) / 2; p.h[p.levels] = (p.h[p.levels - 1] + 1) / 2;
        ++p.levels;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    for (int l = 0; l < p.levels; ++l) {
        const size_t n = (size_t)p.w[l] * p.h[l];
        p.pyr_a[l] = take(n * 4); p.pyr_b[l] = take(n * 4);
        p.flow0[l] = l ? take(n * 8) : 0; p.flow1[l] = take(n * 8);
    }
    p.coef = take((size_t)W * H * 16);
    p.bytes = off;
    return FAV_OK;
}

}  // namespace

extern "C" size_t fav_flow_workspace_bytes(int W, int H, const fav_flow_opts* opts_host)
{
    FlowPlan p;
    return make_plan(W, H, opts_host, p) ? 0 : p.bytes;
}

extern "C" int fav_flow_rgb8(const uint8_t* a_rgb_hwc, const uint8_t* b_rgb_hwc, int W, int H, const fav_flow_opts* opts_host, float* flow_out,
                             void* workspace, size_t workspace_bytes, fav_hipstream_t stream)
{
    FlowPlan p;
    int rc = make_plan(W, H, opts_host, p); if (rc) return rc;
    FAV_REQUIRE(a_rgb_hwc && b_rgb_hwc && flow_out && workspace, "fav_flow_rgb8: null pointer");
    FAV_REQUIRE(workspace_bytes >= p.bytes, "fav_flow_rgb8: the workspace holds %zu bytes, fav_flow_workspace_bytes asks for %zu", workspace_bytes, p.bytes);
    FAV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && reinterpret_cast<uintptr_t>(flow_out) % 8 == 0, "fav_flow_rgb8: the workspace must be 16-byte aligned, flow_out 8-byte aligned");
    rc = ensure_device(); if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    auto f = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    float* coef = f(p.coef);

    // grey + pyramids
    const uint8_t* img[2] = {a_rgb_hwc, b_rgb_hwc};
    for (int k = 0; k < 2; ++k) {
        const size_t* pyr = k ? p.pyr_b : p.pyr_a;
        rc = launch_flow_grey(img[k], f(pyr[0]), W, H, st); if (rc) return rc;
        for (int l = 1; l < p.levels; ++l) { rc = launch_flow_down(f(pyr[l - 1]), p.w[l - 1], p.h[l - 1], f(pyr[l]), st); if (rc) return rc; }
    }
    // coarse to fine.  Every warp ends ceil(iters / K) buffer swaps later: level 0 starts in the buffer that leaves the result in flow_out
    const int swaps = p.warps * ((p.iters + p.K - 1) / p.K);
    const float* coarser = nullptr;
    for (int l = p.levels - 1; l >= 0; --l) {
        float* cur = l ? f(p.flow0[l]) : flow_out;
        float* other = f(p.flow1[l]);
        if (l == 0 && (swaps & 1)) std::swap(cur, other);
        const int w = p.w[l], h = p.h[l];
        if (!coarser) FAV_HIP(hipMemsetAsync(cur, 0, (size_t)w * h * 8, st));
        else { rc = launch_flow_up(coarser, p.w[l + 1], p.h[l + 1], cur, w, h, st); if (rc) return rc; }
        for (int k = 0; k < p.warps; ++k) {
            rc = launch_flow_coef(f(p.pyr_a[l]), f(p.pyr_b[l]), cur, p.alpha, coef, w, h, st); if (rc) return rc;
            rc = launch_flow_sweeps(&cur, &other, coef, p.iters, p.K, w, h, st); if (rc) return rc;
        }
        coarser = cur;
    }
    return FAV_OK;
}

// ---- the stages on their own (tests: each is held to tests/util/flow_model.py)
extern "C" int fav_flow_grey_f32(const uint8_t* rgb_hwc, float* grey, int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(rgb_hwc && grey && W > 0 && H > 0, "fav_flow_grey_f32: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_grey(rgb_hwc, grey, W, H, static_cast<hipStream_t>(stream));
}

extern "C" int fav_flow_down_f32(const float* src, float* dst, int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(src && dst && W > 0 && H > 0, "fav_flow_down_f32: bad argument");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_down(src, W, H, dst, static_cast<hipStream_t>(stream));
}

extern "C" int fav_flow_up_f32(const float* coarse_flow, int Wc, int Hc, float* fine_flow, int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(coarse_flow && fine_flow && Wc > 0 && Hc > 0 && W > 0 && H > 0, "fav_flow_up_f32: bad argument");
    FAV_REQUIRE(reinterpret_cast<uintptr_t>(coarse_flow) % 8 == 0 && reinterpret_cast<uintptr_t>(fine_flow) % 8 == 0, "fav_flow_up_f32: flows must be 8-byte aligned");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_up(coarse_flow, Wc, Hc, fine_flow, W, H, static_cast<hipStream_t>(stream));
}

extern "C" int fav_flow_coefficients_f32(const float* a_grey, const float* b_grey, const float* flow0, float alpha, float* coef, int W, int H,
                                         fav_hipstream_t stream)
{
    FAV_REQUIRE(a_grey && b_grey && flow0 && coef && W > 0 && H > 0 && std::isfinite(alpha) && alpha > 0.f, "fav_flow_coefficients_f32: bad argument");
    FAV_REQUIRE(reinterpret_cast<uintptr_t>(flow0) % 8 == 0 && reinterpret_cast<uintptr_t>(coef) % 16 == 0, "fav_flow_coefficients_f32: flow0 must be 8-byte aligned, coef 16-byte aligned");
    int rc = ensure_device(); if (rc) return rc;
    return launch_flow_coef(a_grey, b_grey, flow0, alpha, coef, W, H, static_cast<hipStream_t>(stream));
}

extern "C" int fav_flow_sweeps_f32(const float* flow0, const float* coef, int iters, int sweeps_per_launch, float* flow_out, float* scratch,
                                   int W, int H, fav_hipstream_t stream)
{
    FAV_REQUIRE(flow0 && coef && flow_out && scratch && W > 0 && H > 0, "fav_flow_sweeps_f32: bad argument");
    FAV_REQUIRE(iters >= 1 && sweeps_per_launch >= 0 && sweeps_per_launch <= FLOW_MAX_SWEEPS_PER_LAUNCH, "fav_flow_sweeps_f32: iters must be >= 1, sweeps_per_launch 0 (default) .. %d", FLOW_MAX_SWEEPS_PER_LAUNCH);
    FAV_REQUIRE(reinterpret_cast<uintptr_t>(flow0) % 8 == 0 && reinterpret_cast<uintptr_t>(flow_out) % 8 == 0 && reinterpret_cast<uintptr_t>(scratch) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(coef) % 16 == 0, "fav_flow_sweeps_f32: flows must be 8-byte aligned, coef 16-byte aligned");
    int rc = ensure_device(); if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int K = sweeps_per_launch ? sweeps_per_launch : DEFAULT_SWEEPS_PER_LAUNCH;
    // flow0 is read only: the first launch goes from it into the buffer from which the remaining launches end in flow_out
    const int first = std::min(K, iters), rest_launches = (iters - first + K - 1) / K;
    float* src = const_cast<float*>(flow0);
    float* cur = (rest_launches & 1) ? scratch : flow_out;
    float* other = (rest_launches & 1) ? flow_out : scratch;
    float* first_dst = cur;
    rc = launch_flow_sweeps(&src, &first_dst, coef, first, K, W, H, st); if (rc) return rc;
    if (iters > first) { rc = launch_flow_sweeps(&cur, &other, coef, iters - first, K, W, H, st); if (rc) return rc; }
    return FAV_OK;
}
