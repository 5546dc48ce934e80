"""-scale_factor without a GPU: the flag contract of fav_stylize (fast_artistic_video.lua:35, core.lua:127-130) and sanity checks of
the numpy restatement of image.scale(.., 'bicubic') (tests/util/bicubic_model.py) that the GPU tests of the resampling rest on."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import bicubic_model as M  # noqa: E402

EXE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
FLAGS = ["-input_pattern", "x", "-flow_pattern", "a", "-occlusions_pattern", "b"]


def test_scale_factor_is_accepted(favlib):
    r = subprocess.run([EXE] + FLAGS + ["-scale_factor", "0.5", "-dry_run", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("value", ["0", "-1", "abc"])
def test_scale_factor_must_be_a_positive_number(favlib, value):
    r = subprocess.run([EXE] + FLAGS + ["-scale_factor", value, "-dry_run", "1"], capture_output=True, text=True)
    assert r.returncode != 0 and "-scale_factor" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_copies_equal_sizes_and_keeps_the_last_samples(dtype):
    rng = np.random.default_rng(1)
    src = rng.random((3, 9, 14), dtype=np.float32)
    assert np.array_equal(M.scale(src, 9, 14, dtype), src.astype(dtype))
    for hd, wd in [(4, 6), (9, 30), (23, 14), (17, 5)]:
        d = M.scale(src, hd, wd, dtype)
        assert d.shape == (3, hd, wd) and d.dtype == dtype
        if wd == 14: assert np.array_equal(d[:, -1, :], src[:, -1, :].astype(dtype))      # equal-width axis: the last row is the source's
        if hd == 9: assert np.array_equal(d[:, :, -1], src[:, :, -1].astype(dtype))
        assert np.array_equal(d[:, -1, -1], src[:, -1, -1].astype(dtype))
    # last row / column of a resampled axis: the source's last row / column resampled along the other axis alone
    d = M.scale(src, 5, 20, dtype)
    assert np.array_equal(d[:, -1:, :], M.scale(src[:, -1:, :], 1, 20, dtype))
    assert np.array_equal(d[:, :, -1:], M.scale(src[:, :, -1:], 5, 1, dtype))
    # a one-sample source axis is repeated
    assert np.array_equal(M.scale(src[:, :1, :], 4, 14, dtype), np.repeat(src[:, :1, :].astype(dtype), 4, axis=1))


@pytest.mark.parametrize("shape", [((7, 11), (15, 5)), ((7, 11), (3, 29)), ((2, 2), (5, 5)), ((2, 9), (6, 4)), ((64, 48), (23, 101))])
def test_model_reproduces_a_linear_ramp(shape):
    """Catmull-Rom with linearly extrapolated ends is exact on affine data: a*x + b*y + c comes back at every destination sample, the
    borders (and a 2-sample axis, where both extrapolations act at once) included"""
    (hs, ws), (hd, wd) = shape
    a, b, c = 0.75, -1.5, 3.0                                           # (exactly representable: the source ramp itself is exact in fp32)
    y, x = np.mgrid[0:hs, 0:ws]
    src = (a * x + b * y + c).astype(np.float32)[None]
    # destination sample (dy, dx) sits at the fp32 position the definition gives it; the last sample at the source's last
    def pos(n_src, n_dst):
        p = (np.arange(n_dst, dtype=np.float32) * (np.float32(n_src - 1) / np.float32(n_dst - 1))).astype(np.float64)
        p[-1] = n_src - 1
        return p
    want = a * pos(ws, wd)[None, :] + b * pos(hs, hd)[:, None] + c
    mag = np.abs(src).max()
    assert np.abs(M.scale(src, hd, wd, np.float64)[0] - want).max() <= 8 * np.finfo(np.float64).eps * mag
    assert np.abs(M.scale(src, hd, wd, np.float32)[0] - want).max() <= 8 * np.finfo(np.float32).eps * mag      # a few ulp of the ramp's range


def test_model_two_sample_axis():
    src = np.array([[[1.0, 3.0]]], np.float32)                          # p0 = 2*1 - 3 = -1, p3 = 2*3 - 1 = 5: the cubic is the line
    assert np.array_equal(M.scale(src, 1, 5, np.float32), np.array([[[1.0, 1.5, 2.0, 2.5, 3.0]]], np.float32))
    assert np.array_equal(M.scale(np.swapaxes(src, 1, 2), 5, 1, np.float32), np.array([[[1.0], [1.5], [2.0], [2.5], [3.0]]], np.float32))


@pytest.mark.parametrize("k", range(len(M.CASES)))
def test_float32_model_stays_close_to_the_float64_model(k):
    _, _, _, hd, wd = M.CASES[k]
    for src in M.case_inputs(k):
        e32 = np.abs(M.scale(src, hd, wd, np.float32).astype(np.float64) - M.scale(src, hd, wd, np.float64)).max()
        print(f"case {M.CASES[k]} max|src| {np.abs(src).max():.4g}: max|M32 - M64| = {e32:.3e} (bound {2.0 ** -20 * np.abs(src).max():.3e})")
        assert e32 <= 2.0 ** -20 * np.abs(src).max()
