// kernels_flow.hip -- dense optical flow for gfx950: Horn-Schunck with warping, coarse to fine, Jacobi sweeps ("fav_flow";
// restated in numpy by tests/util/flow_model.py, which these kernels follow bit for bit in fp32).
//
// Flow "from A to B" is w with B(p + w(p)) ~ A(p); flows are the .flo payload [H][W][2] (u, v).
//   grey          g = (0.299 R + 0.587 G) + 0.114 B on the bytes
//   down          [1 2 1]/4 along x, then along y (borders replicated, each pass rounded), then the 2x2 mean -> ceil(w/2) x ceil(h/2)
//   up_flow       bilinear at ((x + 0.5) / 2 - 0.5, (y + 0.5) / 2 - 0.5) clamped to the coarse grid; u * (w / wc), v * (h / hc)
//   coefficients  Bw = B(p + w0) bilinear with clamped coordinates; a = Ix, b = Iy central differences of Bw * 0.5 (borders replicated);
//                 c = (Bw - A) - a u0 - b v0;  r = 1 / (alpha^2 + a^2 + b^2)  -> float4 (a, b, c, r) per pixel
//   sweep         u_bar, v_bar = 4-neighbour means (borders replicated); t = (a u_bar + b v_bar + c) r;  u = u_bar - a t, v = v_bar - b t
// Edge-preserving smoothness (smooth_eps > 0; restated by tests/util/flow_robust_model.py), per warp from its starting flow w0, fixed for
// all its sweeps:
//   diffusivity   g = 1 / sqrt(((u_x^2 + v_x^2) + (u_y^2 + v_y^2)) + eps^2), central differences * 0.5 of w0, borders replicated
//   edge weights  w_q = 0.5 (g_p + g_q), q = left, right, up, down (index clamped to the image);  S = (w_l + w_r) + (w_u + w_d)
//                 r = 1 / (((alpha^2 S) 0.25 + a^2) + b^2);  stored: n_q = w_q / S -> float4 (n_l, n_r, n_u, n_d) per pixel
//   sweep         u_bar = (n_l u_l + n_r u_r) + (n_u u_u + n_d u_d), v_bar likewise; the rest as above
//
// The sweeps are the hot path: iters x warps x levels x 2 directions of them per frame.  One sweep per launch is a pass over HBM of
// 32 bytes per pixel; flow_sweep_kernel runs up to K sweeps per launch on a tile that lives in LDS (temporal blocking).  Jacobi reads
// the previous sweep only, so the result does not depend on K or on the tiling.
// Compiled with -ffp-contract=off: every operation rounds like the CPU restatement.
//
// Every kernel is batched: blockIdx.z is the ITEM (an image for grey / down, a flow for up / coefficients / sweeps), all items of a launch
// have one size, and an item's planes are found through FlowPtrs tables that travel BY VALUE in the kernel arguments (<= 16 pointers each,
// read with scalar loads; no table in device memory, so a call needs no copy and may run on two streams at once).  The per-pixel
// arithmetic knows nothing of the batch: an item's bits are those of a launch of its own.
#include <type_traits>

#include "fav_internal.h"

namespace fav {
namespace {

// img [h][w] at (px, py), coordinates clamped to the image: lerp along x in both rows, then along y
__device__ __forceinline__ float bilinear(const float* __restrict__ img, int w, int h, float px, float py)
{
    px = fminf(fmaxf(px, 0.f), (float)(w - 1));
    py = fminf(fmaxf(py, 0.f), (float)(h - 1));
    const float flx = floorf(px), fly = floorf(py);
    const int x0 = (int)flx, y0 = (int)fly;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float fx = px - flx, fy = py - fly;
    const float* r0 = img + (size_t)y0 * w;
    const float* r1 = img + (size_t)y1 * w;
    const float a00 = r0[x0], a01 = r0[x1], a10 = r1[x0], a11 = r1[x1];
    const float top = a00 + fx * (a01 - a00);
    const float bot = a10 + fx * (a11 - a10);
    return top + fy * (bot - top);
}

__global__ __launch_bounds__(256) void flow_grey_kernel(FlowPtrs rgbs, FlowPtrs greys, size_t n)
{
    const uint8_t* __restrict__ rgb = static_cast<const uint8_t*>(rgbs.p[blockIdx.z]);
    float* __restrict__ g = static_cast<float*>(greys.p[blockIdx.z]);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = (float)rgb[i * 3], gr = (float)rgb[i * 3 + 1], b = (float)rgb[i * 3 + 2];
    g[i] = (0.299f * r + 0.587f * gr) + 0.114f * b;
}

// one lane per destination sample: the four blurred samples under it, each from its 3 x 3 neighbourhood (a 4 x 4 gather the L1 serves)
__global__ __launch_bounds__(256) void flow_down_kernel(FlowPtrs srcs, int w, int h, FlowPtrs dsts, int wd, int hd)
{
    const float* __restrict__ src = static_cast<const float*>(srcs.p[blockIdx.z]);
    float* __restrict__ dst = static_cast<float*>(dsts.p[blockIdx.z]);
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= wd || oy >= hd) return;
    auto blur_x = [&](int y, int x) {      // y, x inside the image
        const float* row = src + (size_t)y * w;
        return ((row[max(x - 1, 0)] + 2.f * row[x]) + row[min(x + 1, w - 1)]) * 0.25f;
    };
    auto blur = [&](int y, int x) { return ((blur_x(max(y - 1, 0), x) + 2.f * blur_x(y, x)) + blur_x(min(y + 1, h - 1), x)) * 0.25f; };
    const int x0 = 2 * ox, x1 = min(2 * ox + 1, w - 1), y0 = 2 * oy, y1 = min(2 * oy + 1, h - 1);
    dst[(size_t)oy * wd + ox] = ((blur(y0, x0) + blur(y0, x1)) + (blur(y1, x0) + blur(y1, x1))) * 0.25f;
}

__global__ __launch_bounds__(256) void flow_up_kernel(FlowPtrs coarses, int wc, int hc, FlowPtrs fines, int w, int h, float sx, float sy)
{
    const float2* __restrict__ coarse = static_cast<const float2*>(coarses.p[blockIdx.z]);
    float2* __restrict__ fine = static_cast<float2*>(fines.p[blockIdx.z]);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    float px = ((float)x + 0.5f) * 0.5f - 0.5f, py = ((float)y + 0.5f) * 0.5f - 0.5f;
    px = fminf(fmaxf(px, 0.f), (float)(wc - 1));
    py = fminf(fmaxf(py, 0.f), (float)(hc - 1));
    const float flx = floorf(px), fly = floorf(py);
    const int x0 = (int)flx, y0 = (int)fly;
    const int x1 = min(x0 + 1, wc - 1), y1 = min(y0 + 1, hc - 1);
    const float fx = px - flx, fy = py - fly;
    const float2 a00 = coarse[(size_t)y0 * wc + x0], a01 = coarse[(size_t)y0 * wc + x1];
    const float2 a10 = coarse[(size_t)y1 * wc + x0], a11 = coarse[(size_t)y1 * wc + x1];
    const float tu = a00.x + fx * (a01.x - a00.x), bu = a10.x + fx * (a11.x - a10.x);
    const float tv = a00.y + fx * (a01.y - a00.y), bv = a10.y + fx * (a11.y - a10.y);
    fine[(size_t)y * w + x] = make_float2((tu + fy * (bu - tu)) * sx, (tv + fy * (bv - tv)) * sy);
}

// warp + derivatives + coefficients in one launch: a lane forms Bw at its pixel and at its four (replicated) neighbours -- each with that
// pixel's own flow -- instead of a second pass over a stored Bw.
// ROBUST: the lane also forms the diffusivity g at its pixel and at its four (clamped) neighbours, each from the four neighbours of THAT
// pixel: a 13-point stencil of flow0 that the L1 serves, once per warp.  eps2 = eps^2 (formed on the host in fp32).  The option's arguments
// come last and are an empty struct in the plain instantiation: it reads its arguments where it always has, and a launch carries no
// table it does not use (the estimator is launch-bound).
template <bool ROBUST> struct CoefRobustArgs {};
template <> struct CoefRobustArgs<true> { float eps2; FlowPtrs wgts; };
template <bool ROBUST> struct SweepRobustArgs {};
template <> struct SweepRobustArgs<true> { FlowPtrs wgts; };

// Bw at (xx, yy) inside the image: B at the pixel displaced by its own flow
__device__ __forceinline__ float warped(const float* __restrict__ B, const float2* __restrict__ flow0, int w, int h, int yy, int xx)
{
    const float2 f = flow0[(size_t)yy * w + xx];
    return bilinear(B, w, h, (float)xx + f.x, (float)yy + f.y);
}

// the diffusivity and the four edge weights of pixel (x, y): stores the normalised n_q = w_q / S at wgt and returns S
__device__ __forceinline__ float edge_weights(const float2* __restrict__ flow0, int w, int h, int x, int y, float eps2, float4* wgt)
{
    auto g_at = [&](int yy, int xx) {      // yy, xx inside the image
        const float2 l = flow0[(size_t)yy * w + max(xx - 1, 0)], r = flow0[(size_t)yy * w + min(xx + 1, w - 1)];
        const float2 u = flow0[(size_t)max(yy - 1, 0) * w + xx], d = flow0[(size_t)min(yy + 1, h - 1) * w + xx];
        const float ux = (r.x - l.x) * 0.5f, vx = (r.y - l.y) * 0.5f, uy = (d.x - u.x) * 0.5f, vy = (d.y - u.y) * 0.5f;
        return 1.f / sqrtf(((ux * ux + vx * vx) + (uy * uy + vy * vy)) + eps2);      // sqrt and division correctly rounded, each
    };
    const float gp = g_at(y, x);
    const float wl = 0.5f * (gp + g_at(y, max(x - 1, 0))), wr = 0.5f * (gp + g_at(y, min(x + 1, w - 1)));
    const float wu = 0.5f * (gp + g_at(max(y - 1, 0), x)), wd = 0.5f * (gp + g_at(min(y + 1, h - 1), x));
    const float S = (wl + wr) + (wu + wd);
    *wgt = make_float4(wl / S, wr / S, wu / S, wd / S);
    return S;
}

// (a, b, c) of the brightness term at (x, y): the only statement of the 5-point warp stencil
__device__ __forceinline__ float3 bright_abc(const float* __restrict__ A, const float* __restrict__ B, const float2* __restrict__ flow0, int w, int h, int x, int y)
{
    auto bw = [&](int yy, int xx) { return warped(B, flow0, w, h, yy, xx); };
    const float2 f0 = flow0[(size_t)y * w + x];
    const float bc = bilinear(B, w, h, (float)x + f0.x, (float)y + f0.y);
    const float a = (bw(y, min(x + 1, w - 1)) - bw(y, max(x - 1, 0))) * 0.5f;
    const float b = (bw(min(y + 1, h - 1), x) - bw(max(y - 1, 0), x)) * 0.5f;
    const float it = bc - A[(size_t)y * w + x];
    return make_float3(a, b, (it - a * f0.x) - b * f0.y);
}

template <bool ROBUST>
__global__ __launch_bounds__(256) void flow_coef_kernel(FlowPtrs As, FlowPtrs Bs, FlowPtrs flow0s, float alpha2, FlowPtrs coefs, int w, int h,
                                                        CoefRobustArgs<ROBUST> ra)
{
    const float* __restrict__ A = static_cast<const float*>(As.p[blockIdx.z]);
    const float* __restrict__ B = static_cast<const float*>(Bs.p[blockIdx.z]);
    const float2* __restrict__ flow0 = static_cast<const float2*>(flow0s.p[blockIdx.z]);
    float4* __restrict__ coef = static_cast<float4*>(coefs.p[blockIdx.z]);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const float3 abc = bright_abc(A, B, flow0, w, h, x, y);
    const float a = abc.x, b = abc.y, c = abc.z;
    float wgt = alpha2;
    if constexpr (ROBUST) wgt = (alpha2 * edge_weights(flow0, w, h, x, y, ra.eps2, static_cast<float4*>(ra.wgts.p[blockIdx.z]) + (size_t)y * w + x)) * 0.25f;
    const float r = 1.f / ((wgt + a * a) + b * b);      // one correctly rounded division (-fhip-fp32-correctly-rounded-divide-sqrt)
    coef[(size_t)y * w + x] = make_float4(a, b, c, r);
}

// ---- gradient-constancy data term (fav_flow_opts_ex.data_term = FAV_FLOW_DATA_GRADIENT; restated by tests/util/flow_grad_model.py).
// The data term is taken on (Bx, By) = grad Bw against (Ax, Ay) = grad A instead of Bw against A: two channels k = x, y with
//   a_k = dx(B_k), b_k = dy(B_k), c_k = ((B_k - A_k) - a_k u0) - b_k v0          (dx, dy: central differences * 0.5, borders replicated at
//                                                                                each application)
//   J11 = a_x^2 + a_y^2, J12 = a_x b_x + a_y b_y, J22 = b_x^2 + b_y^2, h1 = a_x c_x + a_y c_y, h2 = b_x c_x + b_y c_y
//   w = alpha^2 | (alpha^2 S) 0.25;  d11 = w + J11, d22 = w + J22, det = d11 d22 - J12^2
//   stored, FIVE PLANES [5][H][W]:  q11 = w d22 / det, q12 = -(w J12 / det), q22 = w d11 / det, e1 = -((d22 h1 - J12 h2) / det),
//                                   e2 = -((d11 h2 - J12 h1) / det)
//   sweep   u = (q11 u_bar + q12 v_bar) + e1, v = (q12 u_bar + q22 v_bar) + e2
// A lane forms Bw on the 13-point diamond of radius 2 around its pixel -- each sample with that pixel's own flow, the L1 serves them --
// and reads A on its cross.  A second difference at the image border nests two clamps: clamp(clamp(x + 1) - 1) is x inside the image and
// x - 1 on its last column, so the sample it needs is one of the 13 either way and is chosen by value.
// The five values are planes, not a record: a wave's loads and stores are 256 contiguous bytes each, and 20 bytes per pixel need no padding.
struct DataTensor { float J11, J12, J22, h1, h2; };

__device__ __forceinline__ DataTensor grad_tensor(const float* __restrict__ A, const float* __restrict__ B, const float2* __restrict__ flow0, int w, int h, int x, int y)
{
    auto bw = [&](int yy, int xx) { return warped(B, flow0, w, h, yy, xx); };
    const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
    const float c0 = bw(y, x);
    const float l1 = bw(y, xm), r1 = bw(y, xp), u1 = bw(ym, x), d1 = bw(yp, x);
    const float l2 = bw(y, max(xm - 1, 0)), r2 = bw(y, min(xp + 1, w - 1)), u2 = bw(max(ym - 1, 0), x), d2 = bw(min(yp + 1, h - 1), x);
    const float ul = bw(ym, xm), ur = bw(ym, xp), dl = bw(yp, xm), dr = bw(yp, xp);
    // Bw at clamp(xm + 1), clamp(xp - 1), clamp(ym + 1), clamp(yp - 1): the centre, or on the image's edge the neighbour on the other side
    const float xm_p = x > 0 ? c0 : r1, xp_m = x < w - 1 ? c0 : l1, ym_p = y > 0 ? c0 : d1, yp_m = y < h - 1 ? c0 : u1;
    const float Bx = (r1 - l1) * 0.5f, By = (d1 - u1) * 0.5f;
    const float Bx_r = (r2 - xp_m) * 0.5f, Bx_l = (xm_p - l2) * 0.5f, Bx_u = (ur - ul) * 0.5f, Bx_d = (dr - dl) * 0.5f;      // Bx at the four neighbours
    const float By_d = (d2 - yp_m) * 0.5f, By_u = (ym_p - u2) * 0.5f, By_l = (dl - ul) * 0.5f, By_r = (dr - ur) * 0.5f;      // By likewise
    const float ax = (Bx_r - Bx_l) * 0.5f, bx = (Bx_d - Bx_u) * 0.5f;
    const float ay = (By_r - By_l) * 0.5f, by = (By_d - By_u) * 0.5f;
    const float Ax = (A[(size_t)y * w + xp] - A[(size_t)y * w + xm]) * 0.5f, Ay = (A[(size_t)yp * w + x] - A[(size_t)ym * w + x]) * 0.5f;
    const float2 f0 = flow0[(size_t)y * w + x];
    const float cx = ((Bx - Ax) - ax * f0.x) - bx * f0.y;
    const float cy = ((By - Ay) - ay * f0.x) - by * f0.y;
    return {ax * ax + ay * ay, ax * bx + ay * by, bx * bx + by * by, ax * cx + ay * cy, bx * cx + by * cy};
}

// the 2 x 2 system of a data tensor and the smoothness weight, solved into the five planes
__device__ __forceinline__ void store_solved(float* __restrict__ coef, size_t n, size_t i, float wgt, const DataTensor& t)
{
    const float d11 = wgt + t.J11, d22 = wgt + t.J22;
    const float det = d11 * d22 - t.J12 * t.J12;
    coef[i] = (wgt * d22) / det;                          // five correctly rounded divisions (-fhip-fp32-correctly-rounded-divide-sqrt)
    coef[n + i] = -((wgt * t.J12) / det);
    coef[2 * n + i] = (wgt * d11) / det;
    coef[3 * n + i] = -((d22 * t.h1 - t.J12 * t.h2) / det);
    coef[4 * n + i] = -((d11 * t.h2 - t.J12 * t.h1) / det);
}

template <bool ROBUST>
__global__ __launch_bounds__(256) void flow_coef_grad_kernel(FlowPtrs As, FlowPtrs Bs, FlowPtrs flow0s, float alpha2, FlowPtrs coefs, int w, int h,
                                                             CoefRobustArgs<ROBUST> ra)
{
    const float* __restrict__ A = static_cast<const float*>(As.p[blockIdx.z]);
    const float* __restrict__ B = static_cast<const float*>(Bs.p[blockIdx.z]);
    const float2* __restrict__ flow0 = static_cast<const float2*>(flow0s.p[blockIdx.z]);
    float* __restrict__ coef = static_cast<float*>(coefs.p[blockIdx.z]);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const DataTensor t = grad_tensor(A, B, flow0, w, h, x, y);
    float wgt = alpha2;
    if constexpr (ROBUST) wgt = (alpha2 * edge_weights(flow0, w, h, x, y, ra.eps2, static_cast<float4*>(ra.wgts.p[blockIdx.z]) + (size_t)y * w + x)) * 0.25f;
    store_solved(coef, (size_t)w * h, (size_t)y * w + x, wgt, t);
}

// ---- the matching prior (fav_flow_opts_ex2.match_beta > 0; DESIGN.md, "Matching prior"; restated by tests/util/flow_match_model.py).
// Block matching at pyramid level 1 on the grey planes rounded to bytes gives an integer displacement d and a confidence m per pixel;
// carried to every level as three planes [3][h][w] = (d.x, d.y, m), it pulls the flow towards d wherever the warp's starting flow is
// further than tau from it:
//   on = max(|d.x - u0|, |d.y - v0|) > tau;  bm = (beta m) on                                  (lagged: fixed for the warp's sweeps)
//   J11 += bm, J22 += bm, h1 -= bm d.x, h2 -= bm d.y       on the data tensor of either data term (brightness: [[a a, a b], [a b, b b]],
//                                                          h = (a c, b c)); then the stored five planes, and the sweep is GradCell's
// Level 0 stores no planes of its own: a lane reads the parent sample (x >> 1, y >> 1) of level 1 and scales d (shift, sx, sy).
//
// flow_match_kernel: cost(p, d) = sum over the 7 x 7 window q around p, q clamped to the image, of |A(q) - B(clamp(q + d))|, minimised
// over d in [-R, R]^2, ties to the first d with dy ascending (outer), dx ascending (inner).  A block owns a tile of 32 x 64 pixels and
// stages, once, the rounded A tile (+ 3 on every side) and the B search window (+ R + 3) in LDS as bytes, both with clamped
// coordinates; a lane owns one column and a run of 8 rows.  Per displacement it forms the 14 row sums of its column position -- each
// one is 7 bytes of A (kept in registers, two packed words) against 7 bytes of B: three aligned LDS words, two v_alignbyte, two v_perm
// and two v_sad_u8 -- and slides the 7-row window down its run: 14 x 7 absolute differences for 8 pixels instead of 8 x 49.  The
// v_perm replicates the image's edge column where the window's q were clamped (the selectors are per lane, fixed for all d).  The
// minimum lives in registers as cost << 13 | index of d, so that one v_min_u32 keeps the first of equal costs; the cost volume never
// leaves the CU.  LDS reads (ds_read_b32: 32 banks, conflicts within a 32-lane half): a half wave is one run of 32 columns, four
// neighbouring lanes share a word (broadcast) and the eight distinct words are consecutive, so every read is conflict-free.
constexpr int MT_W = 32, MT_H = 64, MT_RUN = 8, MT_HALF = 3, MT_ROWS = MT_RUN + 2 * MT_HALF;
constexpr int MT_MAX_R = FLOW_MATCH_MAX_RADIUS;
constexpr int MT_A_PITCH = (MT_W + 2 * MT_HALF + 5 + 3) & ~3;                          // a lane reads 12 bytes from byte lx & ~3 on
constexpr int MT_A_BYTES = (MT_H + 2 * MT_HALF) * MT_A_PITCH;
constexpr int mt_b_pitch(int R) { return (MT_W + 2 * R + 2 * MT_HALF + 5 + 3) & ~3; }   // likewise, from (lx + dx + R) & ~3 on
constexpr int MT_B_BYTES = (MT_H + 2 * MT_MAX_R + 2 * MT_HALF) * mt_b_pitch(MT_MAX_R);

__device__ __forceinline__ uint32_t grey_byte(const float* __restrict__ g, int w, int h, int y, int x)
{
    const float v = g[(size_t)min(max(y, 0), h - 1) * w + min(max(x, 0), w - 1)];
    return (uint32_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
}

// bytes [o, o + 8) of an LDS row given as words, o = 4 wo + s: the low and the high word
__device__ __forceinline__ void eight_bytes(const uint32_t* __restrict__ row, int wo, int s, uint32_t& lo, uint32_t& hi)
{
    const uint32_t w0 = row[wo], w1 = row[wo + 1], w2 = row[wo + 2];
    lo = __builtin_amdgcn_alignbyte(w1, w0, s);
    hi = __builtin_amdgcn_alignbyte(w2, w1, s);
}

__global__ __launch_bounds__(256) void flow_match_kernel(FlowPtrs As, FlowPtrs Bs, FlowPtrs ds, int w, int h, int R)
{
    __shared__ uint32_t sA[MT_A_BYTES / 4];
    __shared__ uint32_t sB[MT_B_BYTES / 4];
    const float* __restrict__ A = static_cast<const float*>(As.p[blockIdx.z]);
    const float* __restrict__ B = static_cast<const float*>(Bs.p[blockIdx.z]);
    short2* __restrict__ dout = static_cast<short2*>(ds.p[blockIdx.z]);
    const int tx0 = blockIdx.x * MT_W, ty0 = blockIdx.y * MT_H;
    const int bpitch = mt_b_pitch(R), bpw = bpitch >> 2, brows = MT_H + 2 * R + 2 * MT_HALF;
    const int wx0 = tx0 - R - MT_HALF, wy0 = ty0 - R - MT_HALF;      // image coordinates of window byte (0, 0)
    // stage: a lane packs four bytes into a word
    for (int i = threadIdx.x; i < MT_A_BYTES / 4; i += 256) {
        const int ry = i / (MT_A_PITCH / 4), cx = (i % (MT_A_PITCH / 4)) * 4;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= grey_byte(A, w, h, ty0 - MT_HALF + ry, tx0 - MT_HALF + cx + k) << (8 * k);
        sA[i] = v;
    }
    for (int i = threadIdx.x; i < brows * bpw; i += 256) {
        const int ry = i / bpw, cx = (i % bpw) * 4;
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= grey_byte(B, w, h, wy0 + ry, wx0 + cx + k) << (8 * k);
        sB[i] = v;
    }
    __syncthreads();
    const int lx = threadIdx.x & (MT_W - 1), run = threadIdx.x / MT_W;
    const int gx = tx0 + lx, gy0 = ty0 + run * MT_RUN;
    const int xe = min(gx, w - 1);                                   // lanes right of the image work on its last column and store nothing
    const int cmin = max(xe - MT_HALF, 0);                           // the window's columns clamp(xe - 3 .. xe + 3) all lie in [cmin, cmin + 6]
    uint32_t sel_lo = 0, sel_hi = 0x0c000000u;                       // v_perm selectors: byte clamp(xe + o) - cmin of the eight; 0x0c = zero
#pragma unroll
    for (int o = 0; o < 7; ++o) {
        const uint32_t pick = (uint32_t)(min(max(xe + o - MT_HALF, 0), w - 1) - cmin);
        if (o < 4) sel_lo |= pick << (8 * o); else sel_hi |= pick << (8 * (o - 4));
    }
    // A: the lane's 14 rows of 7 bytes (the tile was staged with clamped coordinates: columns lx .. lx + 6 are clamp(gx - 3 .. gx + 3))
    uint32_t a_lo[MT_ROWS], a_hi[MT_ROWS];
    int brow[MT_ROWS];                                               // word offset of the lane's B row r at dy = -R
#pragma unroll
    for (int r = 0; r < MT_ROWS; ++r) {
        const int ly = min(gy0 + r, h - 1 + MT_HALF) - ty0;          // staged row of image row clamp(gy0 - 3 + r) (rows below the image: its last)
        eight_bytes(sA + ly * (MT_A_PITCH / 4), lx >> 2, lx & 3, a_lo[r], a_hi[r]);
        a_hi[r] &= 0x00ffffffu;
        const int cy = min(max(gy0 - MT_HALF + r, 0), h - 1);
        brow[r] = (cy - R - wy0) * bpw;
    }
    const int bo0 = cmin - wx0 - R;                                  // byte offset of the lane's eight bytes in a window row at dx = -R
    const int side = 2 * R + 1;
    uint32_t best[MT_RUN];
#pragma unroll
    for (int k = 0; k < MT_RUN; ++k) best[k] = 0xffffffffu;
    for (int dyi = 0; dyi < side; ++dyi) {
        const uint32_t* __restrict__ base = sB + dyi * bpw;
        for (int dxi = 0; dxi < side; ++dxi) {
            const int bo = bo0 + dxi, wo = bo >> 2, s = bo & 3;
            uint32_t hrow[MT_ROWS];
#pragma unroll
            for (int r = 0; r < MT_ROWS; ++r) {
                uint32_t lo, hi;
                eight_bytes(base + brow[r], wo, s, lo, hi);
                const uint32_t plo = __builtin_amdgcn_perm(hi, lo, sel_lo), phi = __builtin_amdgcn_perm(hi, lo, sel_hi);
                hrow[r] = __builtin_amdgcn_sad_u8(plo, a_lo[r], __builtin_amdgcn_sad_u8(phi, a_hi[r], 0u));
            }
            const uint32_t idx = (uint32_t)(dyi * side + dxi);
            uint32_t cost = ((hrow[0] + hrow[1]) + (hrow[2] + hrow[3])) + ((hrow[4] + hrow[5]) + hrow[6]);
#pragma unroll
            for (int k = 0; k < MT_RUN; ++k) {
                if (k) cost = cost + hrow[k + 6] - hrow[k - 1];
                best[k] = min(best[k], (cost << 13) | idx);
            }
        }
    }
    if (gx >= w) return;
#pragma unroll
    for (int k = 0; k < MT_RUN; ++k) {
        const int gy = gy0 + k;
        if (gy < h) {
            const int idx = (int)(best[k] & 0x1fffu);
            dout[(size_t)gy * w + gx] = make_short2((short)(idx % side - R), (short)(idx / side - R));
        }
    }
}

// the forward-backward test of two match fields, and the level-1 prior of the flow "from A to B": planes (d.x, d.y, m), m = 1 when
// t = p + d_AB(p) lies inside the image and max(|d_AB(p) + d_BA(t)|) <= 1
__global__ __launch_bounds__(256) void flow_match_check_kernel(FlowPtrs dabs, FlowPtrs dbas, FlowPtrs priors, int w, int h)
{
    const short2* __restrict__ dab = static_cast<const short2*>(dabs.p[blockIdx.z]);
    const short2* __restrict__ dba = static_cast<const short2*>(dbas.p[blockIdx.z]);
    float* __restrict__ prior = static_cast<float*>(priors.p[blockIdx.z]);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const short2 d = dab[(size_t)y * w + x];
    const int tx = x + d.x, ty = y + d.y;
    float m = 0.f;
    if (tx >= 0 && tx < w && ty >= 0 && ty < h) {
        const short2 b = dba[(size_t)ty * w + tx];
        m = max(abs(d.x + b.x), abs(d.y + b.y)) <= 1 ? 1.f : 0.f;
    }
    const size_t n = (size_t)w * h, i = (size_t)y * w + x;
    prior[i] = (float)d.x; prior[n + i] = (float)d.y; prior[2 * n + i] = m;
}

// the prior of the next coarser level: s = (m00 + m01) + (m10 + m11); m = s 0.25; d = the m-weighted mean times (sx, sy), 0 where s = 0
__global__ __launch_bounds__(256) void flow_prior_down_kernel(FlowPtrs srcs, int w, int h, FlowPtrs dsts, int wd, int hd, float sx, float sy)
{
    const float* __restrict__ src = static_cast<const float*>(srcs.p[blockIdx.z]);
    float* __restrict__ dst = static_cast<float*>(dsts.p[blockIdx.z]);
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= wd || oy >= hd) return;
    const int x0 = 2 * ox, x1 = min(2 * ox + 1, w - 1), y0 = 2 * oy, y1 = min(2 * oy + 1, h - 1);
    const size_t n = (size_t)w * h, i00 = (size_t)y0 * w + x0, i01 = (size_t)y0 * w + x1, i10 = (size_t)y1 * w + x0, i11 = (size_t)y1 * w + x1;
    const float m00 = src[2 * n + i00], m01 = src[2 * n + i01], m10 = src[2 * n + i10], m11 = src[2 * n + i11];
    const float s = (m00 + m01) + (m10 + m11);
    const float tx = (m00 * src[i00] + m01 * src[i01]) + (m10 * src[i10] + m11 * src[i11]);
    const float ty = (m00 * src[n + i00] + m01 * src[n + i01]) + (m10 * src[n + i10] + m11 * src[n + i11]);
    const size_t nd = (size_t)wd * hd, o = (size_t)oy * wd + ox;
    dst[o] = s > 0.f ? (tx / s) * sx : 0.f;
    dst[nd + o] = s > 0.f ? (ty / s) * sy : 0.f;
    dst[2 * nd + o] = s * 0.25f;
}

// the coefficients of a warp with the prior, either data term: always the five planes
template <bool GRAD, bool ROBUST>
__global__ __launch_bounds__(256) void flow_coef_prior_kernel(FlowPtrs As, FlowPtrs Bs, FlowPtrs flow0s, float alpha2, FlowPtrs coefs, int w, int h,
                                                              FlowPrior pr, CoefRobustArgs<ROBUST> ra)
{
    const float* __restrict__ A = static_cast<const float*>(As.p[blockIdx.z]);
    const float* __restrict__ B = static_cast<const float*>(Bs.p[blockIdx.z]);
    const float2* __restrict__ flow0 = static_cast<const float2*>(flow0s.p[blockIdx.z]);
    float* __restrict__ coef = static_cast<float*>(coefs.p[blockIdx.z]);
    const float* __restrict__ prior = static_cast<const float*>(pr.planes.p[blockIdx.z]);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    DataTensor t;
    if constexpr (GRAD) t = grad_tensor(A, B, flow0, w, h, x, y);
    else {
        const float3 abc = bright_abc(A, B, flow0, w, h, x, y);
        t = {abc.x * abc.x, abc.x * abc.y, abc.y * abc.y, abc.x * abc.z, abc.y * abc.z};
    }
    const size_t pn = (size_t)pr.pw * pr.ph, pi = (size_t)min(y >> pr.shift, pr.ph - 1) * pr.pw + min(x >> pr.shift, pr.pw - 1);
    const float dx = prior[pi] * pr.sx, dy = prior[pn + pi] * pr.sy, m = prior[2 * pn + pi];
    const float2 f0 = flow0[(size_t)y * w + x];
    const float on = fmaxf(fabsf(dx - f0.x), fabsf(dy - f0.y)) > pr.tau ? 1.f : 0.f;
    const float bm = (pr.beta * m) * on;
    t.J11 = t.J11 + bm; t.J22 = t.J22 + bm;
    t.h1 = t.h1 - bm * dx; t.h2 = t.h2 - bm * dy;
    float wgt = alpha2;
    if constexpr (ROBUST) wgt = (alpha2 * edge_weights(flow0, w, h, x, y, ra.eps2, static_cast<float4*>(ra.wgts.p[blockIdx.z]) + (size_t)y * w + x)) * 0.25f;
    store_solved(coef, (size_t)w * h, (size_t)y * w + x, wgt, t);
}

// ---- the sweeps, temporally blocked.
// A block owns a REGION of 64 x 64 cells: an interior of (64 - 2K)^2 cells and a halo of K cells around it.  It loads the region's (u, v)
// into LDS (float2, 32 KB) and its coefficients into registers (a lane keeps one column position and ROWS rows, ty + TY j), runs
// n <= K sweeps there and writes the interior.  After sweep s the cells nearer than s to the region's edge are stale; they are never
// written back, and the interior stays s <= K cells away from them.
// Image borders: a neighbour index is clamped to the IMAGE first (then to the region), at every sweep, so the edge cell of the image is
// its own neighbour exactly as in the one-sweep form; region cells outside the image are loaded from clamped addresses, are read by no
// cell inside it and are never stored.
// LDS traffic: a wave reads rows of 64 float2 -- 32 lanes x 8 B = one 256-B bank row per half wave, conflict-free for the centre, left /
// right (shifted by one lane) and up / down (another row) taps alike.  Two barriers per sweep (all new values are formed in registers
// before any is stored), one buffer: 32 KB per block.
// The data term is the CELL: what a lane keeps per cell next to the flow, how it is loaded, and the update from the neighbour mean.
// WEIGHTED: the weighted mean of the edge-preserving smoothness; the four normalised weights of a cell travel in registers too.
// Rows per lane: the brightness cell with the plain mean takes 16 (64 VGPRs of coefficients, 256 lanes per block); with the weights that
// would be 128 VGPRs of coefficients and one wave per SIMD, so every other instantiation runs 512 lanes per block and 8 rows per lane --
// the same region, the same LDS layout and barriers, half the cells per lane (the figures are in DESIGN.md).
constexpr int SW_R = 64;           // region side

// brightness constancy: (a, b, c, r) of flow_coef_kernel;  t = ((a u_bar + b v_bar) + c) r;  u = u_bar - a t, v = v_bar - b t
struct BrightCell {
    static constexpr int rows(bool weighted) { return weighted ? 8 : 16; }
    float4 cf;
    __device__ __forceinline__ void load(const void* __restrict__ coef, size_t idx, size_t) { cf = static_cast<const float4*>(coef)[idx]; }
    __device__ __forceinline__ float2 update(float ub, float vb) const
    {
        const float t = ((cf.x * ub + cf.y * vb) + cf.z) * cf.w;
        return make_float2(ub - cf.x * t, vb - cf.y * t);
    }
};

// gradient constancy, the tensor form: the five planes of flow_coef_grad_kernel
struct GradCell {
    static constexpr int rows(bool) { return 8; }
    float q11, q12, q22, e1, e2;
    __device__ __forceinline__ void load(const void* __restrict__ coef, size_t idx, size_t plane)
    {
        const float* __restrict__ c = static_cast<const float*>(coef);
        q11 = c[idx]; q12 = c[plane + idx]; q22 = c[2 * plane + idx]; e1 = c[3 * plane + idx]; e2 = c[4 * plane + idx];
    }
    __device__ __forceinline__ float2 update(float ub, float vb) const { return make_float2((q11 * ub + q12 * vb) + e1, (q12 * ub + q22 * vb) + e2); }
};

// (u_bar, v_bar) of a cell from its four neighbours; wt is read only when WEIGHTED
template <bool WEIGHTED>
__device__ __forceinline__ float2 neighbour_mean(const float4& wt, float2 L, float2 R, float2 U, float2 D)
{
    if constexpr (WEIGHTED) return make_float2((wt.x * L.x + wt.y * R.x) + (wt.z * U.x + wt.w * D.x), (wt.x * L.y + wt.y * R.y) + (wt.z * U.y + wt.w * D.y));
    else return make_float2(((L.x + R.x) + (U.x + D.x)) * 0.25f, ((L.y + R.y) + (U.y + D.y)) * 0.25f);
}

template <class Cell, bool WEIGHTED>
struct SweepShape {
    static constexpr int ROWS = Cell::rows(WEIGHTED);  // rows per lane
    static constexpr int TY = SW_R / ROWS;             // lanes per column: 64 columns x TY lanes
    static constexpr int THREADS = SW_R * TY;          // 256 | 512
};

template <class Cell, bool WEIGHTED>
__global__ __launch_bounds__((SweepShape<Cell, WEIGHTED>::THREADS)) void flow_sweep_kernel(FlowPtrs fins, FlowPtrs coefs, FlowPtrs fouts, int W, int H, int K, int n,
                                                                                         SweepRobustArgs<WEIGHTED> ra)
{
    constexpr int ROWS = SweepShape<Cell, WEIGHTED>::ROWS, TY = SweepShape<Cell, WEIGHTED>::TY;
    __shared__ float2 s[SW_R][SW_R];
    const float2* __restrict__ fin = static_cast<const float2*>(fins.p[blockIdx.z]);
    const void* __restrict__ coef = coefs.p[blockIdx.z];
    float2* __restrict__ fout = static_cast<float2*>(fouts.p[blockIdx.z]);
    const size_t plane = (size_t)W * H;
    const int lx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int TI = SW_R - 2 * K;
    const int x0 = (int)blockIdx.x * TI - K, y0 = (int)blockIdx.y * TI - K;
    const int gx = x0 + lx;
    const int cx = min(max(gx, 0), W - 1);
    const int lxl = (gx > 0 && lx > 0) ? lx - 1 : lx;
    const int lxr = (gx < W - 1 && lx < SW_R - 1) ? lx + 1 : lx;
    Cell cell[ROWS];
    float4 wt[WEIGHTED ? ROWS : 1];
    float2 nv[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int ly = ty + TY * j;
        const int cy = min(max(y0 + ly, 0), H - 1);
        const size_t idx = (size_t)cy * W + cx;
        cell[j].load(coef, idx, plane);
        if constexpr (WEIGHTED) wt[j] = static_cast<const float4*>(ra.wgts.p[blockIdx.z])[idx];
        s[ly][lx] = fin[idx];
    }
    __syncthreads();
    for (int sweep = 0; sweep < n; ++sweep) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int ly = ty + TY * j, gy = y0 + ly;
            const int lyu = (gy > 0 && ly > 0) ? ly - 1 : ly;
            const int lyd = (gy < H - 1 && ly < SW_R - 1) ? ly + 1 : ly;
            const float2 m = neighbour_mean<WEIGHTED>(wt[WEIGHTED ? j : 0], s[ly][lxl], s[ly][lxr], s[lyu][lx], s[lyd][lx]);
            nv[j] = cell[j].update(m.x, m.y);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < ROWS; ++j) s[ty + TY * j][lx] = nv[j];
        __syncthreads();
    }
    if (lx < K || lx >= SW_R - K || gx >= W) return;      // (gx >= 0 here: lx >= K)
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int ly = ty + TY * j, gy = y0 + ly;
        if (ly >= K && ly < SW_R - K && gy < H) fout[(size_t)gy * W + gx] = s[ly][lx];
    }
}

// ---- median filtering of the flow between warps (fav_flow_opts_ex3.median = 3 | 5; DESIGN.md, "Median filtering"; restated by
// tests/util/flow_median_model.py).  After the sweeps of a warp u and v are replaced, each on its own, by the median of their
// (2R + 1)^2 window, R = median / 2, neighbour indices clamped to the image.  Nothing is computed, only selected: the result equals
// a sort's middle element value for value.
// A block owns a tile of 64 x 16 pixels and stages it with a halo of R (coordinates clamped to the image: the replicated border) in
// LDS as float2; a lane owns one column and the rows ty + 4 j.  Per pixel it reads its window -- a wave is one row of 64 columns, so
// at any window offset and any row pitch consecutive lanes read consecutive float2: the 32 lanes of a ds_read_b64's conflict group
// cover 256 contiguous bytes, all 64 banks once, and the 16 lanes of a group of ds_read2_b64 (what the compiler makes of two taps)
// 128 contiguous bytes, its 32 banks once: conflict-free either way, no padding -- and runs a fixed selection network on it in
// registers, first for u, then for v: 19 compare-exchanges for 9 values,
// 99 for 25 (the classical median networks; every table below sorts all 2^n inputs of zeros and ones to the right middle wire,
// which by the 0-1 principle is every input).  The tables are unrolled, so every array index is a constant and nothing goes to scratch.
// A compare-exchange is a permutation of its two inputs (a < b picks both sides), so no value is duplicated or lost, -0 / +0 included.
constexpr int MED_TW = 64, MED_TH = 16, MED_TY = 4;
constexpr unsigned char MED9_NET[19][2] = {{1, 2}, {4, 5}, {7, 8}, {0, 1}, {3, 4}, {6, 7}, {1, 2}, {4, 5}, {7, 8}, {0, 3}, {5, 8}, {4, 7}, {3, 6}, {1, 4}, {2, 5},
                                           {4, 7}, {4, 2}, {6, 4}, {4, 2}};
constexpr unsigned char MED25_NET[99][2] = {
    {0, 1}, {3, 4}, {2, 4}, {2, 3}, {6, 7}, {5, 7}, {5, 6}, {9, 10}, {8, 10}, {8, 9}, {12, 13}, {11, 13}, {11, 12}, {15, 16}, {14, 16}, {14, 15}, {18, 19},
    {17, 19}, {17, 18}, {21, 22}, {20, 22}, {20, 21}, {23, 24}, {2, 5}, {3, 6}, {0, 6}, {0, 3}, {4, 7}, {1, 7}, {1, 4}, {11, 14}, {8, 14}, {8, 11}, {12, 15},
    {9, 15}, {9, 12}, {13, 16}, {10, 16}, {10, 13}, {20, 23}, {17, 23}, {17, 20}, {21, 24}, {18, 24}, {18, 21}, {19, 22}, {8, 17}, {9, 18}, {0, 18}, {0, 9},
    {10, 19}, {1, 19}, {1, 10}, {11, 20}, {2, 20}, {2, 11}, {12, 21}, {3, 21}, {3, 12}, {13, 22}, {4, 22}, {4, 13}, {14, 23}, {5, 23}, {5, 14}, {15, 24},
    {6, 24}, {6, 15}, {7, 16}, {7, 19}, {13, 21}, {15, 23}, {7, 13}, {7, 15}, {1, 9}, {3, 11}, {5, 17}, {11, 17}, {9, 17}, {4, 10}, {6, 12}, {7, 14}, {4, 6},
    {4, 7}, {12, 14}, {10, 14}, {6, 7}, {10, 12}, {6, 10}, {6, 17}, {12, 17}, {7, 17}, {7, 10}, {12, 18}, {7, 12}, {10, 18}, {12, 20}, {10, 20}, {10, 12}};

// the smaller of the two into a, the larger into b
__device__ __forceinline__ void compare_exchange(float& a, float& b)
{
    const bool lt = a < b;
    const float lo = lt ? a : b, hi = lt ? b : a;
    a = lo; b = hi;
}

// the middle element of p's (2R + 1)^2 values (p is permuted)
template <int R>
__device__ __forceinline__ float median_select(float (&p)[(2 * R + 1) * (2 * R + 1)])
{
    static_assert(R == 1 || R == 2, "a 3 x 3 or a 5 x 5 window");
    if constexpr (R == 1) {
#pragma unroll
        for (int i = 0; i < 19; ++i) compare_exchange(p[MED9_NET[i][0]], p[MED9_NET[i][1]]);
        return p[4];
    } else {
#pragma unroll
        for (int i = 0; i < 99; ++i) compare_exchange(p[MED25_NET[i][0]], p[MED25_NET[i][1]]);
        return p[12];
    }
}

template <int R>
__global__ __launch_bounds__(256) void flow_median_kernel(FlowPtrs srcs, FlowPtrs dsts, int w, int h)
{
    constexpr int S = 2 * R + 1, COLS = MED_TW + 2 * R, ROWS = MED_TH + 2 * R;
    __shared__ float2 s[ROWS][COLS];
    const float2* __restrict__ src = static_cast<const float2*>(srcs.p[blockIdx.z]);
    float2* __restrict__ dst = static_cast<float2*>(dsts.p[blockIdx.z]);
    const int tx0 = blockIdx.x * MED_TW, ty0 = blockIdx.y * MED_TH;
    for (int i = threadIdx.x; i < ROWS * COLS; i += 256) {
        const int ry = i / COLS, cx = i - ry * COLS;
        const int cy = min(max(ty0 - R + ry, 0), h - 1), ccx = min(max(tx0 - R + cx, 0), w - 1);
        s[ry][cx] = src[(size_t)cy * w + ccx];
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ty = threadIdx.x >> 6, gx = tx0 + lx;
    if (gx >= w) return;
#pragma unroll
    for (int j = 0; j < MED_TH / MED_TY; ++j) {
        const int ly = ty + MED_TY * j, gy = ty0 + ly;
        if (gy < h) {
            float u[S * S], v[S * S];      // window sample (dy, dx) is staged cell (ly + dy, lx + dx)
#pragma unroll
            for (int dy = 0; dy < S; ++dy)
#pragma unroll
                for (int dx = 0; dx < S; ++dx) {
                    const float2 t = s[ly + dy][lx + dx];
                    u[dy * S + dx] = t.x; v[dy * S + dx] = t.y;
                }
            const float mu = median_select<R>(u), mv = median_select<R>(v);
            dst[(size_t)gy * w + gx] = make_float2(mu, mv);
        }
    }
}

// the one place that maps a variant to an instantiation: f(grad, weighted, prior), three std::bool_constant
template <class F>
void with_variant(const FlowVariant& v, F&& f)
{
    auto prior = [&](auto grad, auto weighted) { if (v.prior) f(grad, weighted, std::true_type{}); else f(grad, weighted, std::false_type{}); };
    auto weighted = [&](auto grad) { if (v.wgt) prior(grad, std::true_type{}); else prior(grad, std::false_type{}); };
    if (v.grad) weighted(std::true_type{}); else weighted(std::false_type{});
}

inline dim3 grid_64x4(int w, int h, int items) { return dim3((w + 63) / 64, (h + 3) / 4, items); }
inline bool size_ok(int w, int h) { return w > 0 && h > 0 && (long long)w * h <= (1ll << 28) && (h + 3) / 4 <= 65535; }
inline bool items_ok(int items) { return items >= 1 && items <= FLOW_MAX_ITEMS; }

}  // namespace

int launch_flow_grey(const FlowPtrs& rgb_hwc, const FlowPtrs& grey, int items, int W, int H, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && items_ok(items), "flow grey: bad size %dx%d x %d", W, H, items);
    const size_t n = (size_t)W * H;
    hipLaunchKernelGGL(flow_grey_kernel, dim3((unsigned)((n + 255) / 256), 1, items), dim3(256), 0, st, rgb_hwc, grey, n);
    FAV_LAUNCH_CHECK("flow_grey_kernel");
    return FAV_OK;
}

int launch_flow_down(const FlowPtrs& src, int W, int H, const FlowPtrs& dst, int items, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && items_ok(items), "flow down: bad size %dx%d x %d", W, H, items);
    const int wd = (W + 1) / 2, hd = (H + 1) / 2;
    hipLaunchKernelGGL(flow_down_kernel, grid_64x4(wd, hd, items), dim3(256), 0, st, src, W, H, dst, wd, hd);
    FAV_LAUNCH_CHECK("flow_down_kernel");
    return FAV_OK;
}

int launch_flow_up(const FlowPtrs& coarse, int Wc, int Hc, const FlowPtrs& fine, int items, int W, int H, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && size_ok(Wc, Hc) && items_ok(items), "flow up: bad size %dx%d -> %dx%d x %d", Wc, Hc, W, H, items);
    hipLaunchKernelGGL(flow_up_kernel, grid_64x4(W, H, items), dim3(256), 0, st, coarse, Wc, Hc, fine, W, H, (float)W / (float)Wc, (float)H / (float)Hc);
    FAV_LAUNCH_CHECK("flow_up_kernel");
    return FAV_OK;
}

int launch_flow_coef(const FlowPtrs& A, const FlowPtrs& B, const FlowPtrs& flow0, const FlowPtrs& coef, const FlowVariant& v, int items, int W, int H, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && items_ok(items), "flow coefficients: bad size %dx%d x %d", W, H, items);
    with_variant(v, [&](auto grad, auto weighted, auto prior) {
        constexpr bool GRAD = decltype(grad)::value, ROBUST = decltype(weighted)::value;
        CoefRobustArgs<ROBUST> ra;
        if constexpr (ROBUST) ra = {v.eps * v.eps, *v.wgt};
        if constexpr (decltype(prior)::value)
            hipLaunchKernelGGL((flow_coef_prior_kernel<GRAD, ROBUST>), grid_64x4(W, H, items), dim3(256), 0, st, A, B, flow0, v.alpha * v.alpha, coef, W, H, *v.prior, ra);
        else
            hipLaunchKernelGGL(GRAD ? flow_coef_grad_kernel<ROBUST> : flow_coef_kernel<ROBUST>, grid_64x4(W, H, items), dim3(256), 0, st, A, B, flow0,
                               v.alpha * v.alpha, coef, W, H, ra);
    });
    FAV_LAUNCH_CHECK("flow_coef_kernel");
    return FAV_OK;
}

int launch_flow_match(const FlowPtrs& A, const FlowPtrs& B, const FlowPtrs& d, int items, int W, int H, int radius, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && items_ok(items) && radius >= 1 && radius <= FLOW_MATCH_MAX_RADIUS, "flow match: bad argument (%dx%d x %d, radius %d)", W, H, items, radius);
    const dim3 grid((W + MT_W - 1) / MT_W, (H + MT_H - 1) / MT_H, items);
    FAV_REQUIRE(grid.y <= 65535, "flow match: %d rows are too many", H);
    hipLaunchKernelGGL(flow_match_kernel, grid, dim3(256), 0, st, A, B, d, W, H, radius);
    FAV_LAUNCH_CHECK("flow_match_kernel");
    return FAV_OK;
}

int launch_flow_match_check(const FlowPtrs& d_ab, const FlowPtrs& d_ba, const FlowPtrs& prior, int items, int W, int H, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && items_ok(items), "flow match check: bad size %dx%d x %d", W, H, items);
    hipLaunchKernelGGL(flow_match_check_kernel, grid_64x4(W, H, items), dim3(256), 0, st, d_ab, d_ba, prior, W, H);
    FAV_LAUNCH_CHECK("flow_match_check_kernel");
    return FAV_OK;
}

int launch_flow_prior_down(const FlowPtrs& src, int W, int H, const FlowPtrs& dst, int items, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && items_ok(items), "flow prior down: bad size %dx%d x %d", W, H, items);
    const int wd = (W + 1) / 2, hd = (H + 1) / 2;
    hipLaunchKernelGGL(flow_prior_down_kernel, grid_64x4(wd, hd, items), dim3(256), 0, st, src, W, H, dst, wd, hd, (float)wd / (float)W, (float)hd / (float)H);
    FAV_LAUNCH_CHECK("flow_prior_down_kernel");
    return FAV_OK;
}

// `iters` sweeps from *cur, ceil(iters / K) launches between *cur and *other (every item at once); on return *cur holds the results
int launch_flow_sweeps(FlowPtrs* cur, FlowPtrs* other, const FlowPtrs& coef, const FlowVariant& v, int items, int iters, int K, int W, int H, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && items_ok(items) && iters >= 1 && K >= 1 && K <= FLOW_MAX_SWEEPS_PER_LAUNCH,
                "flow sweeps: bad argument (%dx%d x %d, %d sweeps, %d per launch)", W, H, items, iters, K);
    const int ti = SW_R - 2 * K;
    const dim3 grid((W + ti - 1) / ti, (H + ti - 1) / ti, items);
    FAV_REQUIRE(grid.y <= 65535, "flow sweeps: %d rows are too many", H);
    for (int done = 0; done < iters; done += K) {
        with_variant(v, [&](auto grad, auto weighted, auto prior) {
            constexpr bool WEIGHTED = decltype(weighted)::value;
            using Cell = std::conditional_t<decltype(grad)::value || decltype(prior)::value, GradCell, BrightCell>;      // (with the prior: the five planes)
            SweepRobustArgs<WEIGHTED> ra;
            if constexpr (WEIGHTED) ra = {*v.wgt};
            hipLaunchKernelGGL((flow_sweep_kernel<Cell, WEIGHTED>), grid, dim3(SweepShape<Cell, WEIGHTED>::THREADS), 0, st, *cur, coef, *other, W, H, K,
                               std::min(K, iters - done), ra);
        });
        FAV_LAUNCH_CHECK("flow_sweep_kernel");
        std::swap(*cur, *other);
    }
    return FAV_OK;
}

// the size x size median (size 3 | 5) of every item's u and v, from src into dst (never in place)
int launch_flow_median(const FlowPtrs& src, const FlowPtrs& dst, int items, int W, int H, int size, hipStream_t st)
{
    FAV_REQUIRE(size_ok(W, H) && items_ok(items) && (size == 3 || size == 5), "flow median: bad argument (%dx%d x %d, window %d)", W, H, items, size);
    for (int j = 0; j < items; ++j) FAV_REQUIRE(src.p[j] && dst.p[j] && src.p[j] != dst.p[j], "flow median: item %d is filtered in place or missing", j);
    const dim3 grid((W + MED_TW - 1) / MED_TW, (H + MED_TH - 1) / MED_TH, items);
    FAV_REQUIRE(grid.y <= 65535, "flow median: %d rows are too many", H);
    hipLaunchKernelGGL(size == 3 ? flow_median_kernel<1> : flow_median_kernel<2>, grid, dim3(256), 0, st, src, dst, W, H);
    FAV_LAUNCH_CHECK("flow_median_kernel");
    return FAV_OK;
}

}  // namespace fav
