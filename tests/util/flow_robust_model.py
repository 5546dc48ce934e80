"""The edge-preserving smoothness option of the optical-flow estimator (fav_flow_opts.smooth_eps > 0; DESIGN.md, "fav_flow", "Edge-
preserving smoothness") restated in numpy, written from its description and not from the kernels it checks.  Everything that the option
does not touch -- grey, pyramid, upsampling, warping, (a, b, c) -- is flow_model's.

Per warp, from the warp's starting flow w0 = (u0, v0), fixed for all its sweeps (lagged diffusivity):
  g    = 1 / sqrt((((u_x^2 + v_x^2) + (u_y^2 + v_y^2)) + eps^2)),  u_x ... central differences x 0.5 of w0, borders replicated
  w_q  = 0.5 (g_p + g_q) towards the four neighbours q = left, right, up, down (index clamped to the image);  S = (w_l + w_r) + (w_u + w_d)
  r    = 1 / (((alpha^2 S) 0.25 + a^2) + b^2)
  n_q  = w_q / S                                  THE STORED FORM: the four weights already divided by S, [H][W][4] = (n_l, n_r, n_u, n_d)
  sweep: u_bar = ((n_l u_l + n_r u_r) + (n_u u_u + n_d u_d)), v_bar likewise;  t = ((a u_bar + b v_bar) + c) r;  u = u_bar - a t, v = v_bar - b t
With g == 1 everywhere: w_q = 1, S = 4, n_q = 0.25, r = 1 / ((alpha^2 + a^2) + b^2) -- flow_model's estimator, so alpha keeps its meaning.

`dtype` as in flow_model: float32 rounds every operation in the order written, float64 is the reference."""
import numpy as np

import flow_model as M

ALPHA, EPS = 5.0, 0.3          # the defaults when the option is on (alpha: when the caller leaves it 0)


def diffusivity(flow0, eps, dtype=np.float32):
    """g [H][W] of the flow w0"""
    k = dtype
    f = np.asarray(flow0, dtype)
    dx = (M._shift(f, 1, 1) - M._shift(f, -1, 1)) * k(0.5)          # (u_x, v_x)
    dy = (M._shift(f, 1, 0) - M._shift(f, -1, 0)) * k(0.5)          # (u_y, v_y)
    s = ((dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]) + (dy[..., 0] * dy[..., 0] + dy[..., 1] * dy[..., 1])) + k(eps) * k(eps)
    g = k(1) / np.sqrt(s)
    assert g.dtype == dtype
    return g


def edge_weights(g, dtype=np.float32):
    """(w [H][W][4] = (w_l, w_r, w_u, w_d), S [H][W]) of a diffusivity image"""
    k = dtype
    g = np.asarray(g, dtype)
    w = np.stack([k(0.5) * (g + M._shift(g, -1, 1)), k(0.5) * (g + M._shift(g, 1, 1)),
                  k(0.5) * (g + M._shift(g, -1, 0)), k(0.5) * (g + M._shift(g, 1, 0))], -1)
    S = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
    return w, S


def coefficients(A, B, flow0, alpha=ALPHA, eps=EPS, dtype=np.float32, g=None):
    """(coef [H][W][4] = (a, b, c, r), weights [H][W][4] = (n_l, n_r, n_u, n_d)) of one warp around flow0; `g` replaces the diffusivity
    (tests: a constant one must give flow_model's estimator back)"""
    k = dtype
    coef = M.coefficients(A, B, flow0, alpha, dtype).copy()
    a, b = coef[..., 0], coef[..., 1]
    w, S = edge_weights(diffusivity(flow0, eps, dtype) if g is None else g, dtype)
    coef[..., 3] = k(1) / ((((k(alpha) * k(alpha)) * S) * k(0.25) + a * a) + b * b)
    n = w / S[..., None]
    assert coef.dtype == dtype and n.dtype == dtype
    return coef, n


def sweeps(flow, coef, weights, n, dtype=np.float32):
    """n weighted Jacobi sweeps over the whole flow"""
    f = np.asarray(flow, dtype).copy(); coef = np.asarray(coef, dtype); wt = np.asarray(weights, dtype)
    a, b, c, r = (coef[..., i] for i in range(4))
    nl, nr, nu, nd = (wt[..., i, None] for i in range(4))
    for _ in range(n):
        m = (nl * M._shift(f, -1, 1) + nr * M._shift(f, 1, 1)) + (nu * M._shift(f, -1, 0) + nd * M._shift(f, 1, 0))
        t = ((a * m[..., 0] + b * m[..., 1]) + c) * r
        f = np.stack([m[..., 0] - a * t, m[..., 1] - b * t], -1)
    assert f.dtype == dtype
    return f


def flow(a_rgb, b_rgb, levels=0, warps=0, iters=0, alpha=0.0, eps=EPS, dtype=np.float32, g=None):
    """the whole estimator with the option on (eps > 0); 0 = default for the others.  `g`: a function (h, w) -> diffusivity image that
    replaces the computed one"""
    assert eps > 0
    warps, iters, alpha = warps or M.WARPS, iters or M.ITERS, alpha or ALPHA
    pa, pb = M.pyramid(a_rgb, levels, dtype), M.pyramid(b_rgb, levels, dtype)
    f = None
    for A, B in zip(pa[::-1], pb[::-1]):
        h, w = A.shape
        f = np.zeros((h, w, 2), dtype) if f is None else M.up_flow(f, h, w, dtype)
        for _ in range(warps):
            coef, wt = coefficients(A, B, f, alpha, eps, dtype, None if g is None else g(h, w))
            f = sweeps(f, coef, wt, iters, dtype)
    return f


# ---- the two-motion scene shared by tests/test_cpu_flow_robust.py and tests/test_gpu_flow_robust.py
FG, BG = (-3.0, 1.5), (2.0, 0.0)          # motion of the rectangle and of the background, px
SCENES = [(96, 128, 1), (96, 128, 2), (150, 203, 1), (150, 203, 2)]          # (h, w, seed)


def _shifted(a, d):
    """a(q - d): Catmull-Rom along x, then along y (flow_model._cubic_axis), fp64"""
    h, w = a.shape[:2]
    return M._cubic_axis(M._cubic_axis(a, np.arange(w) - d[0], 1), np.arange(h) - d[1], 0)


def two_motion_scene(h, w, seed, fg=FG, bg=BG):
    """(A, B, truth [H][W][2], valid [H][W]): a textured rectangle [h//4, 3h//4) x [w//4, 3w//4) moving by `fg` over a background moving
    by `bg`.  truth is the flow from A to B; valid excludes the occluded pixels: background whose rounded target lies under the shifted
    rectangle."""
    from fav_amd import synth
    t1 = synth.smooth_frame(h, w, seed).astype(np.float64)
    t2 = synth.smooth_frame(h, w, seed + 7)[::-1, ::-1].astype(np.float64)
    mask = np.zeros((h, w)); mask[h // 4:3 * h // 4, w // 4:3 * w // 4] = 1.0
    A = np.where(mask[..., None] > 0.5, t2, t1)
    mb = _shifted(mask, fg) > 0.5
    B = np.where(mb[..., None], _shifted(t2, fg), _shifted(t1, bg))
    truth = np.where(mask[..., None] > 0.5, np.array(fg), np.array(bg))
    ys, xs = np.mgrid[0:h, 0:w]
    tx = np.clip(np.rint(xs + bg[0]).astype(np.int64), 0, w - 1); ty = np.clip(np.rint(ys + bg[1]).astype(np.int64), 0, h - 1)
    valid = ~((mask < 0.5) & mb[ty, tx])
    to_u8 = lambda x: np.clip(np.rint(x), 0, 255).astype(np.uint8)
    return to_u8(A), to_u8(B), truth, valid


def scene_epe(f, truth, valid, border=12):
    """mean endpoint error over the non-occluded pixels, `border` px of frame edge excluded"""
    e = np.sqrt(((np.asarray(f, np.float64) - truth) ** 2).sum(-1))[border:-border, border:-border]
    return float(e[valid[border:-border, border:-border]].mean())
