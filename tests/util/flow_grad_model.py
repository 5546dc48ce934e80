"""The gradient-constancy data term of the optical-flow estimator (fav_flow_opts_ex.data_term = FAV_FLOW_DATA_GRADIENT; DESIGN.md,
"fav_flow", "Gradient-constancy data term") restated in numpy, written from its description and not from the kernels it checks.
Everything that the option does not touch -- grey, pyramid, upsampling, warping -- is flow_model's, and the edge weights of
smooth_eps > 0 are flow_robust_model's.

The data term compares the image GRADIENTS instead of the grey levels (Brox et al. 2004), so a change of exposure between the two frames
-- a gain and an offset, slowly varying -- is no longer read as motion.  Per warp around w0 = (u0, v0), with
dx(f) = (f(x + 1) - f(x - 1)) 0.5, dy likewise, borders replicated at EACH application:
  Bw = warp(B, w0);  Bx = dx(Bw), By = dy(Bw);  Ax = dx(A), Ay = dy(A)
  channel x:  a_x = dx(Bx), b_x = dy(Bx), it_x = Bx - Ax          channel y:  a_y = dx(By), b_y = dy(By), it_y = By - Ay
  each:       c = ((it - a u0) - b v0)
  J11 = a_x a_x + a_y a_y,  J12 = a_x b_x + a_y b_y,  J22 = b_x b_x + b_y b_y,  h1 = a_x c_x + a_y c_y,  h2 = b_x c_x + b_y c_y
  w   = alpha alpha                              (quadratic smoothness)
  w   = ((alpha alpha) S) 0.25                   (smooth_eps > 0: S and the stored n_q of flow_robust_model, unchanged)
  d11 = w + J11,  d22 = w + J22,  det = d11 d22 - J12 J12
  THE STORED FORM, five values per pixel and no division left in the sweep:
  q11 = (w d22) / det,  q12 = -((w J12) / det),  q22 = (w d11) / det,  e1 = -((d22 h1 - J12 h2) / det),  e2 = -((d11 h2 - J12 h1) / det)
  sweep: u = ((q11 u_bar + q12 v_bar) + e1),  v = ((q12 u_bar + q22 v_bar) + e2);  u_bar, v_bar: the plain 4-neighbour mean of flow_model
  or the weighted mean of flow_robust_model
(the minimiser of  sum_k (a_k u + b_k v + c_k)^2 + w ((u - u_bar)^2 + (v - v_bar)^2)  over (u, v): a 2 x 2 system solved per pixel).

`dtype` as in flow_model: float32 rounds every operation in the order written, float64 is the reference."""
import numpy as np

import flow_model as M
import flow_robust_model as R

ALPHA, ALPHA_ROBUST = 8.0, 8.0          # the defaults when the caller leaves alpha 0: quadratic smoothness | with smooth_eps > 0


def _dx(f, k):
    return (M._shift(f, 1, 1) - M._shift(f, -1, 1)) * k(0.5)


def _dy(f, k):
    return (M._shift(f, 1, 0) - M._shift(f, -1, 0)) * k(0.5)


def channels(A, B, flow0, dtype=np.float32):
    """((a_x, b_x, c_x), (a_y, b_y, c_y)) of one warp around flow0"""
    k = dtype
    A = np.asarray(A, dtype); flow0 = np.asarray(flow0, dtype)
    u0, v0 = flow0[..., 0], flow0[..., 1]
    bw = M.warp(B, flow0, dtype)
    out = []
    for d in (_dx, _dy):
        g = d(bw, k)
        a, b = _dx(g, k), _dy(g, k)
        it = g - d(A, k)
        out.append((a, b, (it - a * u0) - b * v0))
    return tuple(out)


def stored_form(J11, J12, J22, h1, h2, w):
    """[H][W][5] = (q11, q12, q22, e1, e2) of a data tensor and the smoothness weight w (an array or a scalar of the arithmetic's type)"""
    d11 = w + J11; d22 = w + J22
    det = d11 * d22 - J12 * J12
    return np.stack([(w * d22) / det, -((w * J12) / det), (w * d11) / det, -((d22 * h1 - J12 * h2) / det), -((d11 * h2 - J12 * h1) / det)], -1)


def coefficients(A, B, flow0, alpha=ALPHA, eps=0.0, dtype=np.float32):
    """one warp around flow0 -> coef [H][W][5] (eps == 0) or (coef, weights [H][W][4] = (n_l, n_r, n_u, n_d)) (eps > 0)"""
    k = dtype
    (ax, bx, cx), (ay, by, cy) = channels(A, B, flow0, dtype)
    J11 = ax * ax + ay * ay; J12 = ax * bx + ay * by; J22 = bx * bx + by * by
    h1 = ax * cx + ay * cy; h2 = bx * cx + by * cy
    if eps > 0:
        wq, S = R.edge_weights(R.diffusivity(flow0, eps, dtype), dtype)
        w = ((k(alpha) * k(alpha)) * S) * k(0.25)
    else:
        w = k(alpha) * k(alpha)
    coef = stored_form(J11, J12, J22, h1, h2, w)
    assert coef.dtype == dtype
    if eps > 0:
        n = wq / S[..., None]
        assert n.dtype == dtype
        return coef, n
    return coef


def sweeps(flow, coef, n, dtype=np.float32, weights=None):
    """n Jacobi sweeps of the tensor form over the whole flow; weights: the [H][W][4] of the weighted mean, None for the plain mean"""
    k = dtype
    f = np.asarray(flow, dtype).copy(); coef = np.asarray(coef, dtype)
    q11, q12, q22, e1, e2 = (coef[..., i] for i in range(5))
    if weights is not None:
        nl, nr, nu, nd = (np.asarray(weights, dtype)[..., i, None] for i in range(4))
    for _ in range(n):
        if weights is None:
            m = ((M._shift(f, -1, 1) + M._shift(f, 1, 1)) + (M._shift(f, -1, 0) + M._shift(f, 1, 0))) * k(0.25)
        else:
            m = (nl * M._shift(f, -1, 1) + nr * M._shift(f, 1, 1)) + (nu * M._shift(f, -1, 0) + nd * M._shift(f, 1, 0))
        ub, vb = m[..., 0], m[..., 1]
        f = np.stack([(q11 * ub + q12 * vb) + e1, (q12 * ub + q22 * vb) + e2], -1)
    assert f.dtype == dtype
    return f


def flow(a_rgb, b_rgb, levels=0, warps=0, iters=0, alpha=0.0, eps=0.0, dtype=np.float32):
    """the whole estimator with the gradient term; 0 = default for levels, warps, iters, alpha; eps > 0: edge-preserving smoothness"""
    warps, iters = warps or M.WARPS, iters or M.ITERS
    alpha = alpha or (ALPHA_ROBUST if eps > 0 else ALPHA)
    pa, pb = M.pyramid(a_rgb, levels, dtype), M.pyramid(b_rgb, levels, dtype)
    f = None
    for A, B in zip(pa[::-1], pb[::-1]):
        h, w = A.shape
        f = np.zeros((h, w, 2), dtype) if f is None else M.up_flow(f, h, w, dtype)
        for _ in range(warps):
            if eps > 0:
                coef, wt = coefficients(A, B, f, alpha, eps, dtype)
            else:
                coef, wt = coefficients(A, B, f, alpha, 0.0, dtype), None
            f = sweeps(f, coef, iters, dtype, wt)
    return f


# ---- relit inputs shared by tests/test_cpu_flow_grad.py and tests/test_gpu_flow_grad.py
PAIRS = [(1, 96, 128), (2, 96, 128), (1, 150, 203)]          # (seed, h, w) of flow_model.shifted_pair
RELIGHTS = [(0.8, 10.0), (0.7, 0.0), (1.0, 25.0)]            # (gain, offset)


def relight(img, gain, offset):
    """clip(rint(gain img + offset)) on the bytes"""
    return np.clip(np.rint(gain * np.asarray(img, np.float64) + offset), 0, 255).astype(np.uint8)
