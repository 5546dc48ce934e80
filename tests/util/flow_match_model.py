"""The block-matching prior of the optical-flow estimator (fav_flow_opts_ex2.match_beta > 0; DESIGN.md, "fav_flow", "Matching prior")
restated in numpy, written from its description and not from the kernels it checks.  Everything that the option does not touch -- grey,
pyramid, upsampling, warping, (a, b, c) -- is flow_model's; the edge weights of smooth_eps > 0 are flow_robust_model's; the gradient
channels and the stored five-value form are flow_grad_model's.

1. Matching, at pyramid level LM = 1, on both grey planes rounded to integers (rint, clamped to 0..255):
     cost(p, d) = sum over the 7 x 7 window q around p, each q clamped to the image first, of |A(q) - B(clamp(q + d))|     (an integer)
     d_AB(p)    = argmin over d in [-R, R]^2, ties to the first d in the order dy ascending (outer), dx ascending (inner)
     d_BA       = the same with A and B exchanged
     m(p)       = 1 when t = p + d_AB(p) lies inside the image and max(|d_AB(p) + d_BA(t)|) <= 1 over both components, else 0
2. Carrying (d, m) to level l:
     coarser:  s = (m00 + m01) + (m10 + m11) over the 2 x 2 block (an odd edge's missing partner is the replicated edge sample);
               m = s 0.25;  d = ((m00 d00 + m01 d01) + (m10 d10 + m11 d11)) / s, times w_c / w (x) or h_c / h (y); 0 where s == 0
     level 0:  the parent sample (x >> 1, y >> 1) of level 1, d times w_0 / w_1 (x) and h_0 / h_1 (y)
3. Per warp around w0 = (u0, v0):
     on = max(|d.x - u0|, |d.y - v0|) > tau_l        (tau = 1 at levels >= 1, 2 at level 0)
     bm = (beta m) on                                lagged like the diffusivity: fixed for all the warp's sweeps
     brightness term:  J11 = a a + bm, J12 = a b, J22 = b b + bm, h1 = a c - bm d.x, h2 = b c - bm d.y
     gradient term:    flow_grad_model's tensor with bm added to J11 and J22 and bm d.x, bm d.y subtracted from h1, h2
     w and the stored form (q11, q12, q22, e1, e2): flow_grad_model.stored_form; the sweeps: flow_grad_model.sweeps

`dtype` as in flow_model: float32 rounds every operation in the order written, float64 is the reference."""
import numpy as np

import flow_grad_model as G
import flow_model as M
import flow_robust_model as R

LM, WINDOW, RADIUS, BETA = 1, 7, 16, 225.0
TAU, TAU0 = 1.0, 2.0          # the gate at levels >= 1 | at level 0


def rounded(grey):
    """a grey plane as integers 0..255"""
    return np.clip(np.rint(np.asarray(grey, np.float64)), 0, 255).astype(np.int64)


def match(A, B, radius=RADIUS):
    """d_AB [h][w][2] = (dx, dy), int64, of two grey planes (any float type: they are rounded first)"""
    a, b = rounded(A), rounded(B)
    h, w = a.shape
    half = WINDOW // 2
    ys, xs = np.arange(h), np.arange(w)
    best = np.full((h, w), np.iinfo(np.int64).max)
    d = np.zeros((h, w, 2), np.int64)
    for dy in range(-radius, radius + 1):
        rows = np.clip(ys + dy, 0, h - 1)
        for dx in range(-radius, radius + 1):
            diff = np.abs(a - b[rows][:, np.clip(xs + dx, 0, w - 1)])          # |A(q) - B(clamp(q + d))| for q in the image
            p = np.pad(diff, half, mode="edge")                                 # q clamped to the image: replicated
            c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), 0), 1)
            cost = c[WINDOW:, WINDOW:] - c[:-WINDOW, WINDOW:] - c[WINDOW:, :-WINDOW] + c[:-WINDOW, :-WINDOW]
            better = cost < best
            best[better] = cost[better]
            d[better] = (dx, dy)
    return d


def check(d_ab, d_ba):
    """m [h][w] (0 | 1, float64) of the forward-backward test"""
    h, w, _ = d_ab.shape
    ys, xs = np.mgrid[0:h, 0:w]
    tx, ty = xs + d_ab[..., 0], ys + d_ab[..., 1]
    inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    back = d_ba[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]
    return (inside & (np.abs(d_ab + back).max(-1) <= 1)).astype(np.float64)


def prior_down(d, m, dtype=np.float32):
    """(d, m) of a level -> of the next coarser one"""
    k = dtype
    d = np.asarray(d, dtype); m = np.asarray(m, dtype)
    h, w = m.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    y0 = np.arange(hc) * 2; y1 = np.minimum(y0 + 1, h - 1)
    x0 = np.arange(wc) * 2; x1 = np.minimum(x0 + 1, w - 1)
    pick = lambda a, y, x: a[y][:, x]
    m00, m01, m10, m11 = pick(m, y0, x0), pick(m, y0, x1), pick(m, y1, x0), pick(m, y1, x1)
    s = (m00 + m01) + (m10 + m11)
    out = np.zeros((hc, wc, 2), dtype)
    safe = np.where(s > 0, s, k(1))
    for c, ratio in ((0, k(wc) / k(w)), (1, k(hc) / k(h))):
        dc = d[..., c]
        t = (m00 * pick(dc, y0, x0) + m01 * pick(dc, y0, x1)) + (m10 * pick(dc, y1, x0) + m11 * pick(dc, y1, x1))
        out[..., c] = np.where(s > 0, (t / safe) * ratio, k(0))
    mc = s * k(0.25)
    assert out.dtype == dtype and mc.dtype == dtype
    return out, mc


def prior_level0(d1, m1, h, w, dtype=np.float32):
    """(d, m) of level 1 -> of level 0 (h x w): the parent sample, d scaled by the size ratios"""
    k = dtype
    d1 = np.asarray(d1, dtype); m1 = np.asarray(m1, dtype)
    h1, w1 = m1.shape
    ys, xs = np.mgrid[0:h, 0:w]
    d = d1[ys >> 1, xs >> 1] * np.array([k(w) / k(w1), k(h) / k(h1)], dtype)
    assert d.dtype == dtype
    return d, m1[ys >> 1, xs >> 1]


def prior_pyramid(d_ab, m_ab, sizes, dtype=np.float32):
    """[(d_l, m_l)] for every level of `sizes` (flow_model.level_sizes) from the level-LM match field"""
    assert len(sizes) > LM and tuple(m_ab.shape) == tuple(sizes[LM])
    out = [None] * len(sizes)
    out[LM] = (np.asarray(d_ab, dtype), np.asarray(m_ab, dtype))
    for l in range(LM + 1, len(sizes)):
        out[l] = prior_down(*out[l - 1], dtype)
    out[0] = prior_level0(*out[LM], *sizes[0], dtype)
    return out


def gate(d, flow0, tau, dtype=np.float32):
    """on [H][W] (bool) and the distance it thresholds"""
    d = np.asarray(d, dtype); flow0 = np.asarray(flow0, dtype)
    dist = np.maximum(np.abs(d[..., 0] - flow0[..., 0]), np.abs(d[..., 1] - flow0[..., 1]))
    return dist > dtype(tau), dist


def coefficients(A, B, flow0, d, m, alpha, beta=BETA, tau=TAU, eps=0.0, grad=False, dtype=np.float32):
    """one warp around flow0 with the prior (d, m) of its level -> coef [H][W][5] (eps == 0) or (coef, weights [H][W][4]) (eps > 0)"""
    k = dtype
    d = np.asarray(d, dtype); flow0 = np.asarray(flow0, dtype)
    on, _ = gate(d, flow0, tau, dtype)
    bm = (k(beta) * np.asarray(m, dtype)) * on.astype(dtype)
    if grad:
        (ax, bx, cx), (ay, by, cy) = G.channels(A, B, flow0, dtype)
        J11 = ax * ax + ay * ay; J12 = ax * bx + ay * by; J22 = bx * bx + by * by
        h1 = ax * cx + ay * cy; h2 = bx * cx + by * cy
    else:
        c4 = M.coefficients(A, B, flow0, alpha, dtype)
        a, b, c = c4[..., 0], c4[..., 1], c4[..., 2]
        J11 = a * a; J12 = a * b; J22 = b * b; h1 = a * c; h2 = b * c
    J11 = J11 + bm; J22 = J22 + bm
    h1 = h1 - bm * d[..., 0]; h2 = h2 - bm * d[..., 1]
    if eps > 0:
        wq, S = R.edge_weights(R.diffusivity(flow0, eps, dtype), dtype)
        w = ((k(alpha) * k(alpha)) * S) * k(0.25)
    else:
        w = k(alpha) * k(alpha)
    coef = G.stored_form(J11, J12, J22, h1, h2, w)
    assert coef.dtype == dtype
    if eps > 0:
        n = wq / S[..., None]
        return coef, n
    return coef


def default_alpha(eps, grad):
    return (G.ALPHA_ROBUST if eps > 0 else G.ALPHA) if grad else (R.ALPHA if eps > 0 else M.ALPHA)


def flow(a_rgb, b_rgb, levels=0, warps=0, iters=0, alpha=0.0, eps=0.0, grad=False, beta=BETA, radius=RADIUS, dtype=np.float32, trace=None):
    """the whole estimator with the prior; 0 = default for levels, warps, iters, alpha.  trace: a list that receives the gate distance
    [H][W] of every warp with its tau, in the order of the warps (tests: the fp32 and fp64 models must agree on the gate)"""
    warps, iters = warps or M.WARPS, iters or M.ITERS
    alpha = alpha or default_alpha(eps, grad)
    pa, pb = M.pyramid(a_rgb, levels, dtype), M.pyramid(b_rgb, levels, dtype)
    assert len(pa) > LM, "the prior needs a pyramid of at least two levels"
    d_ab, d_ba = match(pa[LM], pb[LM], radius), match(pb[LM], pa[LM], radius)
    prior = prior_pyramid(d_ab, check(d_ab, d_ba), [g.shape for g in pa], dtype)
    f = None
    for l in range(len(pa) - 1, -1, -1):
        A, B = pa[l], pb[l]
        h, w = A.shape
        f = np.zeros((h, w, 2), dtype) if f is None else M.up_flow(f, h, w, dtype)
        tau = TAU0 if l == 0 else TAU
        for _ in range(warps):
            if trace is not None:
                trace.append((gate(prior[l][0], f, tau, dtype)[1], tau))
            r = coefficients(A, B, f, prior[l][0], prior[l][1], alpha, beta, tau, eps, grad, dtype)
            coef, wt = r if eps > 0 else (r, None)
            f = G.sweeps(f, coef, iters, dtype, wt)
    return f


# ---- the scenes shared by tests/test_cpu_flow_match.py and tests/test_gpu_flow_match.py: flow_robust_model.two_motion_scene with a free
# rectangle.  (seed, (y0, y1, x0, x1), fg motion, bg motion) at 192 x 256
SCENE_H, SCENE_W = 192, 256
LARGE = [(1, (84, 108, 116, 140), (22.0, -14.0), (2.0, 0.0)),
         (2, (60, 90, 150, 180), (-26.0, 9.0), (1.0, -1.5)),
         (3, (70, 118, 40, 88), (30.0, 20.0), (-1.5, 0.5))]
SMALL = (1, (48, 144, 64, 192), (-3.0, 1.5), (2.0, 0.0))
HALF_RECT = (38, 58, 54, 74)


def scene(h, w, seed, rect, fg, bg):
    """(A, B, truth [H][W][2], valid [H][W], object [H][W]): the textured rectangle [y0, y1) x [x0, x1) moving by `fg` over a background
    moving by `bg`; valid excludes the background pixels that the moved rectangle covers"""
    from fav_amd import synth
    y0, y1, x0, x1 = rect
    t1 = synth.smooth_frame(h, w, seed).astype(np.float64)
    t2 = synth.smooth_frame(h, w, seed + 7)[::-1, ::-1].astype(np.float64)
    mask = np.zeros((h, w)); mask[y0:y1, x0:x1] = 1.0
    obj = mask > 0.5
    A = np.where(obj[..., None], t2, t1)
    mb = R._shifted(mask, fg) > 0.5
    B = np.where(mb[..., None], R._shifted(t2, fg), R._shifted(t1, bg))
    truth = np.where(obj[..., None], np.array(fg), np.array(bg))
    ys, xs = np.mgrid[0:h, 0:w]
    tx = np.clip(np.rint(xs + bg[0]).astype(np.int64), 0, w - 1); ty = np.clip(np.rint(ys + bg[1]).astype(np.int64), 0, h - 1)
    valid = ~(~obj & mb[ty, tx])
    to_u8 = lambda x: np.clip(np.rint(x), 0, 255).astype(np.uint8)
    return to_u8(A), to_u8(B), truth, valid, obj


def scene_errors(f, truth, valid, obj, border=12):
    """(mean endpoint error on the object, on the non-occluded background), `border` px of frame edge excluded"""
    e = np.sqrt(((np.asarray(f, np.float64) - truth) ** 2).sum(-1))[border:-border, border:-border]
    o = obj[border:-border, border:-border]; v = valid[border:-border, border:-border]
    return float(e[o].mean()), float(e[v & ~o].mean())


def half_scene():
    """scene 1 at 96 x 128 with both motions halved (the GPU suite's recovery scene, R = 8): fg (11, -7), bg (1, 0).  The rectangle is
    20 x 20 around the halved centre, not 12 x 12: at level 1 a 6 x 6 object is smaller than the 7 x 7 window (measured with the fp64
    models, object error plain -> prior: 12 x 12 15.06 -> 9.55 px, 20 x 20 16.06 -> 4.35 px)"""
    seed, _, fg, bg = LARGE[0]
    return scene(96, 128, seed, HALF_RECT, (fg[0] / 2, fg[1] / 2), (bg[0] / 2, bg[1] / 2))
