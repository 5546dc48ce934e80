"""Median filtering of the flow between warps (fav_flow_opts_ex3.median = 3 | 5; DESIGN.md, "fav_flow", "Median filtering") restated in
numpy, written from its description and not from the kernel it checks.  Every stage of a warp is another model's -- grey, pyramid,
upsampling, the plain coefficients and sweeps: flow_model; the edge weights of smooth_eps > 0: flow_robust_model; the gradient channels
and the stored five-value form: flow_grad_model; the matching prior: flow_match_model -- and only the level / warp loop is restated here,
with the filter in it.

With r = median // 2, after the `iters` sweeps of EVERY warp at EVERY level (the last warp of level 0 included):
  u(p) <- the middle element of the sorted (2r + 1)^2 values u(q), q = p + (dx, dy), |dx|, |dy| <= r, each index clamped to the image
  v(p) <- likewise, on its own
(the 5th smallest of 9, the 13th smallest of 25).  The filtered flow is the w0 of the next warp -- of its coefficients, its diffusivity and
the prior's gate --, what the next finer level upsamples, and at level 0 the result.  Nothing is computed, only selected, so the filter is
the same in every arithmetic; `dtype` is that of the stages around it, as in flow_model."""
import numpy as np

import flow_grad_model as G
import flow_match_model as P
import flow_model as M
import flow_robust_model as R


def median(flow, size):
    """[H][W][C] -> [H][W][C]: every channel's size x size median (size 3 | 5), neighbour indices clamped to the image"""
    assert size in (3, 5)
    f = np.asarray(flow)
    h, w = f.shape[:2]
    r = size // 2
    taps = [f[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(np.arange(w) + dx, 0, w - 1)] for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
    out = np.sort(np.stack(taps, 0), axis=0)[size * size // 2]
    assert out.dtype == f.dtype and out.shape == f.shape
    return out


def flow(a_rgb, b_rgb, levels=0, warps=0, iters=0, alpha=0.0, eps=0.0, grad=False, beta=0.0, radius=P.RADIUS, median_size=0, dtype=np.float32):
    """the whole estimator with every option; 0 = default for levels, warps, iters, alpha; eps > 0: edge-preserving smoothness; grad: the
    gradient-constancy data term; beta > 0: the matching prior; median_size 3 | 5: the filter (0: off -- then this is the model of the
    options given, bit for bit)"""
    assert median_size in (0, 3, 5)
    warps, iters = warps or M.WARPS, iters or M.ITERS
    alpha = alpha or P.default_alpha(eps, grad)
    pa, pb = M.pyramid(a_rgb, levels, dtype), M.pyramid(b_rgb, levels, dtype)
    prior = None
    if beta > 0:
        assert len(pa) > P.LM, "the prior needs a pyramid of at least two levels"
        d_ab, d_ba = P.match(pa[P.LM], pb[P.LM], radius), P.match(pb[P.LM], pa[P.LM], radius)
        prior = P.prior_pyramid(d_ab, P.check(d_ab, d_ba), [g.shape for g in pa], dtype)
    f = None
    for l in range(len(pa) - 1, -1, -1):
        A, B = pa[l], pb[l]
        h, w = A.shape
        f = np.zeros((h, w, 2), dtype) if f is None else M.up_flow(f, h, w, dtype)
        for _ in range(warps):
            if prior is not None:
                r = P.coefficients(A, B, f, prior[l][0], prior[l][1], alpha, beta, P.TAU0 if l == 0 else P.TAU, eps, grad, dtype)
                coef, wt = r if eps > 0 else (r, None)
                f = G.sweeps(f, coef, iters, dtype, wt)
            elif grad:
                r = G.coefficients(A, B, f, alpha, eps, dtype)
                coef, wt = r if eps > 0 else (r, None)
                f = G.sweeps(f, coef, iters, dtype, wt)
            elif eps > 0:
                coef, wt = R.coefficients(A, B, f, alpha, eps, dtype)
                f = R.sweeps(f, coef, wt, iters, dtype)
            else:
                f = M.sweeps(f, M.coefficients(A, B, f, alpha, dtype), iters, dtype)
            if median_size:
                f = median(f, median_size)
    assert f.dtype == dtype
    return f
