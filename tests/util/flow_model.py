"""The coarse-to-fine optical-flow estimator of csrc/kernels_flow.hip ("fav_flow") restated in numpy, written from its
description and not from the kernels it checks.  Horn-Schunck with warping, Jacobi sweeps, every stage callable on its own.

Flow "from A to B" is w with B(p + w(p)) ~ A(p); flows are [H][W][2] (u, v), the .flo payload.

`dtype` is the arithmetic: float32 rounds every operation to fp32 in the order written here (the kernels are compiled without
contraction and with a correctly rounded division, so they follow it bit for bit); float64 is the reference the rounding is measured
against.  Every expression below is parenthesised the way it is evaluated."""
import numpy as np

ALPHA, WARPS, ITERS, MAX_LEVELS, MIN_SIDE = 15.0, 3, 30, 6, 16


def grey(rgb_hwc, dtype=np.float32):
    """bytes [H][W][3] -> [H][W]:  (0.299 R + 0.587 G) + 0.114 B  on 0..255"""
    c = dtype
    p = np.asarray(rgb_hwc).astype(dtype)
    return (c(0.299) * p[..., 0] + c(0.587) * p[..., 1]) + c(0.114) * p[..., 2]


def _shift(a, d, axis):
    """a sampled at index + d along axis, borders replicated"""
    n = a.shape[axis]
    return np.take(a, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


def down(img, dtype=np.float32):
    """[h][w] -> [ceil(h/2)][ceil(w/2)]: [1 2 1]/4 along x, then along y (borders replicated, each pass rounded), then the 2x2 mean
    (an odd edge's missing partner is the replicated edge pixel)"""
    c = dtype
    s = np.asarray(img, dtype)
    h, w = s.shape
    bx = ((_shift(s, -1, 1) + c(2) * s) + _shift(s, 1, 1)) * c(0.25)
    b = ((_shift(bx, -1, 0) + c(2) * bx) + _shift(bx, 1, 0)) * c(0.25)
    y0 = np.arange((h + 1) // 2) * 2; y1 = np.minimum(y0 + 1, h - 1)
    x0 = np.arange((w + 1) // 2) * 2; x1 = np.minimum(x0 + 1, w - 1)
    out = ((b[y0][:, x0] + b[y0][:, x1]) + (b[y1][:, x0] + b[y1][:, x1])) * c(0.25)
    assert out.dtype == dtype
    return out


def level_sizes(h, w, levels=0):
    """[(h, w)] from level 0 on: a level is added while its smaller side is still >= 16, at most 6; `levels` > 0 fixes the count"""
    sizes = [(h, w)]
    while (len(sizes) < levels) if levels > 0 else (len(sizes) < MAX_LEVELS and min((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2) >= MIN_SIDE):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def _lerp(a, b, t):
    return a + t * (b - a)


def _axis_taps(pos, n, dtype):
    """clamped position -> (i0, i1, fraction)"""
    pos = np.minimum(np.maximum(pos, dtype(0)), dtype(n - 1))
    i0 = np.floor(pos).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), (pos - i0.astype(dtype)).astype(dtype)


def bilinear(img, px, py, dtype=np.float32):
    """img [h][w] sampled at (px, py), coordinates clamped to the image: rows first (lerp along x), then lerp along y"""
    img = np.asarray(img, dtype)
    h, w = img.shape
    x0, x1, fx = _axis_taps(np.asarray(px, dtype), w, dtype)
    y0, y1, fy = _axis_taps(np.asarray(py, dtype), h, dtype)
    top = _lerp(img[y0, x0], img[y0, x1], fx)
    bot = _lerp(img[y1, x0], img[y1, x1], fx)
    out = _lerp(top, bot, fy)
    assert out.dtype == dtype
    return out


def up_flow(coarse, h, w, dtype=np.float32):
    """coarse [hc][wc][2] -> [h][w][2]: bilinear at ((x + 0.5) / 2 - 0.5, (y + 0.5) / 2 - 0.5) clamped to the coarse grid, then
    u * (w / wc), v * (h / hc) (the ratios formed in `dtype`)"""
    c = dtype
    coarse = np.asarray(coarse, dtype)
    hc, wc, _ = coarse.shape
    px = (np.arange(w, dtype=dtype) + c(0.5)) * c(0.5) - c(0.5)
    py = (np.arange(h, dtype=dtype) + c(0.5)) * c(0.5) - c(0.5)
    px, py = np.broadcast_to(px[None, :], (h, w)), np.broadcast_to(py[:, None], (h, w))
    out = np.empty((h, w, 2), dtype)
    out[..., 0] = bilinear(coarse[..., 0], px, py, dtype) * (c(w) / c(wc))
    out[..., 1] = bilinear(coarse[..., 1], px, py, dtype) * (c(h) / c(hc))
    return out


def warp(img, flow, dtype=np.float32):
    """Bw(p) = img(p + flow(p)), bilinear, clamped"""
    flow = np.asarray(flow, dtype)
    h, w = flow.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    return bilinear(img, xs.astype(dtype) + flow[..., 0], ys.astype(dtype) + flow[..., 1], dtype)


def coefficients(A, B, flow0, alpha=ALPHA, dtype=np.float32):
    """[H][W][4] = (a, b, c, r) of one warp around flow0"""
    k = dtype
    A = np.asarray(A, dtype); flow0 = np.asarray(flow0, dtype)
    bw = warp(B, flow0, dtype)
    a = (_shift(bw, 1, 1) - _shift(bw, -1, 1)) * k(0.5)
    b = (_shift(bw, 1, 0) - _shift(bw, -1, 0)) * k(0.5)
    it = bw - A
    c = (it - a * flow0[..., 0]) - b * flow0[..., 1]
    r = k(1) / ((k(alpha) * k(alpha) + a * a) + b * b)
    out = np.stack([a, b, c, r], -1)
    assert out.dtype == dtype
    return out


def sweeps(flow, coef, n, dtype=np.float32):
    """n Jacobi sweeps over the whole flow"""
    k = dtype
    f = np.asarray(flow, dtype).copy(); coef = np.asarray(coef, dtype)
    a, b, c, r = (coef[..., i] for i in range(4))
    for _ in range(n):
        m = ((_shift(f, -1, 1) + _shift(f, 1, 1)) + (_shift(f, -1, 0) + _shift(f, 1, 0))) * k(0.25)
        t = ((a * m[..., 0] + b * m[..., 1]) + c) * r
        f = np.stack([m[..., 0] - a * t, m[..., 1] - b * t], -1)
    assert f.dtype == dtype
    return f


def pyramid(rgb_hwc, levels=0, dtype=np.float32):
    g = [grey(rgb_hwc, dtype)]
    for _ in level_sizes(*g[0].shape, levels)[1:]:
        g.append(down(g[-1], dtype))
    return g


def flow(a_rgb, b_rgb, levels=0, warps=0, iters=0, alpha=0.0, dtype=np.float32):
    """the whole estimator; 0 = default, each"""
    warps, iters, alpha = warps or WARPS, iters or ITERS, alpha or ALPHA
    pa, pb = pyramid(a_rgb, levels, dtype), pyramid(b_rgb, levels, dtype)
    f = None
    for A, B in zip(pa[::-1], pb[::-1]):
        h, w = A.shape
        f = np.zeros((h, w, 2), dtype) if f is None else up_flow(f, h, w, dtype)
        for _ in range(warps):
            f = sweeps(f, coefficients(A, B, f, alpha, dtype), iters, dtype)
    return f


# ---- inputs shared by tests/test_cpu_flow.py and tests/test_gpu_flow.py
SHIFT = (3.5, -2.25)
SIZES = [(17, 23), (64, 64), (150, 203)]          # (h, w)


def _cubic_axis(a, pos, axis):
    """Catmull-Rom cubic (the kernel of bicubic_model) through a's samples at fractional positions `pos` along axis, indices clamped; fp64"""
    n = a.shape[axis]
    i = np.floor(pos).astype(np.int64); x = pos - i
    p = [np.take(a, np.clip(i + d, 0, n - 1), axis=axis) for d in (-1, 0, 1, 2)]
    shape = [1] * a.ndim; shape[axis] = -1
    x = x.reshape(shape)
    a1 = p[2] - p[0]; a2 = 2 * p[0] - 5 * p[1] + 4 * p[2] - p[3]; a3 = 3 * (p[1] - p[2]) + p[3] - p[0]
    return p[1] + 0.5 * x * (a1 + x * (a2 + x * a3))


def shifted_pair(seed, h=96, w=128):
    """(A, B, w): A = synth.smooth_frame, B(q) = A(q - w) for the constant flow w = SHIFT, resampled in fp64 with the Catmull-Rom cubic
    of the bicubic model (separable, x first, indices clamped) and rounded to bytes"""
    from fav_amd import synth
    A = synth.smooth_frame(h, w, seed)
    a = A.astype(np.float64)
    b = _cubic_axis(a, np.arange(w) - SHIFT[0], 1)
    b = _cubic_axis(b, np.arange(h) - SHIFT[1], 0)
    return A, np.clip(np.rint(b), 0, 255).astype(np.uint8), SHIFT


def interior_epe(f, w, border=12):
    d = np.asarray(f, np.float64)[border:-border, border:-border] - np.asarray(w, np.float64)
    return float(np.sqrt((d ** 2).sum(-1)).mean())


def warped_pair(h, w, seed, std=1.5):
    """(frame k, frame k warped by synth.backward_flow(std) with the fp64 bilinear sampler, rounded to bytes)"""
    from fav_amd import synth
    A = synth.smooth_frame(h, w, seed)
    bwf = synth.backward_flow(h, w, seed + 1, std=std)
    B = np.stack([warp(A[..., c].astype(np.float64), bwf, np.float64) for c in range(3)], -1)
    return A, np.clip(np.rint(B), 0, 255).astype(np.uint8)
