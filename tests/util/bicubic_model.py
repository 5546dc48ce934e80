"""image.scale(src, Wd, Hd, 'bicubic') on float tensors [Torch7 `image`, recalled] restated in numpy: the arithmetic behind
-scale_factor (fast_artistic_video_core.lua:128,151), written from its description and not from the kernels it checks.

Separable: along the width first, into an intermediate [C][Hs][Wd], then along the height.  Along one axis, with src_len source
samples s and dst_len destination samples d:
  * dst_len == src_len: d = s;  src_len == 1: every d equals s[0];
  * otherwise scale = (float)(src_len - 1) / (float)(dst_len - 1), and for di < dst_len - 1: f = di * scale (both in fp32),
    i = (long)f, x = f - i; p1 = s[i], p2 = s[i + 1], p0 = s[i - 1] or 2 p1 - p2 at the left end, p3 = s[i + 2] or 2 p2 - p1 at
    the right end; d[di] = p1 + 0.5 x (a1 + x (a2 + x a3)) with a1 = p2 - p0, a2 = 2 p0 - 5 p1 + 4 p2 - p3, a3 = 3 (p1 - p2) + p3 - p0;
  * d[dst_len - 1] = s[src_len - 1].
The sample POSITIONS (scale, f, i, x) are fp32 in both forms -- they are part of the definition; `dtype` is the arithmetic on the
samples: float32 rounds every operation (and the intermediate) to fp32, float64 is the reference the rounding is measured against."""
import numpy as np


def _axis(s, dst_len, dtype):
    """resample the LAST axis of s to dst_len samples"""
    s = np.asarray(s, dtype)
    src_len = s.shape[-1]
    if dst_len == src_len:
        return s.copy()
    if src_len == 1:
        return np.repeat(s, dst_len, axis=-1)
    d = np.empty(s.shape[:-1] + (dst_len,), dtype)
    if dst_len > 1:
        scale = np.float32(src_len - 1) / np.float32(dst_len - 1)
        f = np.arange(dst_len - 1, dtype=np.float32) * scale
        i = f.astype(np.int64)
        assert f.dtype == np.float32 and i.min() >= 0 and i.max() + 1 < src_len
        x = (f - i.astype(np.float32)).astype(dtype)
        c = dtype
        p1, p2 = s[..., i], s[..., i + 1]
        p0 = np.where(i > 0, s[..., np.maximum(i - 1, 0)], c(2) * p1 - p2)
        p3 = np.where(i + 2 < src_len, s[..., np.minimum(i + 2, src_len - 1)], c(2) * p2 - p1)
        a1 = p2 - p0
        a2 = c(2) * p0 - c(5) * p1 + c(4) * p2 - p3
        a3 = c(3) * (p1 - p2) + p3 - p0
        d[..., :-1] = p1 + c(0.5) * x * (a1 + x * (a2 + x * a3))
        assert d.dtype == dtype and a3.dtype == dtype
    d[..., -1] = s[..., -1]
    return d


def scale(src, Hd, Wd, dtype=np.float32):
    """src [C][Hs][Ws] -> [C][Hd][Wd]"""
    assert dtype in (np.float32, np.float64)
    wide = _axis(src, Wd, dtype)                                       # [C][Hs][Wd], rounded to `dtype`
    return np.ascontiguousarray(np.swapaxes(_axis(np.swapaxes(wide, -1, -2), Hd, dtype), -1, -2))


# the operator cases of the GPU suite: (C, Hs, Ws, Hd, Wd)
CASES = [(3, 8, 12, 4, 6), (3, 5, 7, 13, 9), (1, 2, 2, 5, 5), (3, 1, 9, 4, 9), (2, 40, 56, 40, 28), (3, 67, 131, 33, 64), (3, 270, 480, 135, 240)]


def case_inputs(k):
    """the two inputs of case k: uniform in [0, 1], and the same scaled to +-300"""
    c, hs, ws, _, _ = CASES[k]
    u = np.random.default_rng(100 + k).random((c, hs, ws), dtype=np.float32)
    return [u, ((u - np.float32(0.5)) * np.float32(600)).astype(np.float32)]
