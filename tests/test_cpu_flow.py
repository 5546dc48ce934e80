"""Host side of the optical-flow estimator (no GPU needed): the numpy model's own properties, the premise that the default options
recover a known motion, the flags of bin/fav_flow and fav_stylize -estimate_flow, the exported symbols and the argument checks that
come before any device is touched."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402

from fav_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
FLOW, STYLIZE = os.path.join(BIN, "fav_flow"), os.path.join(BIN, "fav_stylize")


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=60)


# ------------------------------------------------------------------------------------------------ 1. the model
def test_model_constant_image_gives_exactly_zero_flow():
    img = np.full((40, 56, 3), 77, np.uint8)
    for dt in (np.float32, np.float64):
        f = M.flow(img, img, dtype=dt)
        assert f.shape == (40, 56, 2) and f.dtype == dt and not f.any()


def test_model_sweeps_compose():
    rng = np.random.default_rng(5)
    f0 = rng.standard_normal((19, 27, 2)).astype(np.float32)
    A, B = M.grey(synth.smooth_frame(19, 27, 1)), M.grey(synth.smooth_frame(19, 27, 2))
    coef = M.coefficients(A, B, f0)
    step = f0
    for _ in range(7):
        step = M.sweeps(step, coef, 1)
    assert np.array_equal(M.sweeps(f0, coef, 7), step)


def test_model_affine_flow_is_a_fixed_point_of_the_mean_in_the_interior():
    """with a = b = c = 0 a sweep is the 4-neighbour mean: an affine field keeps its interior (fp64: to rounding), the replicated border
    does not"""
    ys, xs = np.mgrid[0:21, 0:33].astype(np.float64)
    f = np.stack([0.25 * xs - 0.5 * ys + 3.0, -0.125 * xs + 0.75 * ys - 1.0], -1)      # (dyadic coefficients: the mean is exact)
    coef = np.zeros((21, 33, 4)); coef[..., 3] = 1.0 / 225.0
    g = M.sweeps(f, coef, 1, np.float64)
    assert np.array_equal(g[1:-1, 1:-1], f[1:-1, 1:-1])
    assert not np.array_equal(g, f)


def test_model_level_sizes():
    assert M.level_sizes(64, 64) == [(64, 64), (32, 32), (16, 16)]
    assert M.level_sizes(17, 23) == [(17, 23)]
    assert M.level_sizes(150, 203) == [(150, 203), (75, 102), (38, 51), (19, 26)]
    assert len(M.level_sizes(720, 1280)) == 6 and len(M.level_sizes(4000, 4000)) == 6
    assert M.level_sizes(64, 64, 2) == [(64, 64), (32, 32)]


# ------------------------------------------------------------------------------------------------ 2. the premise
def test_default_options_recover_a_known_shift():
    """synth.smooth_frame(96, 128, 1) and the same frame shifted by (+3.5, -2.25) px -- resampled in fp64 with the Catmull-Rom cubic of
    the bicubic model (flow_model.shifted_pair), not by a Fourier shift: the frame is not periodic.  Mean endpoint error of the fp64 model
    over the interior (12-pixel border excluded), default options (alpha 15, 3 warps, 30 sweeps): measured 0.066 px for seed 1 (0.098 and
    0.067 for seeds 2 and 3); required <= 0.5 px."""
    A, B, w = M.shifted_pair(1)
    assert A.shape == (96, 128, 3)
    epe = M.interior_epe(M.flow(A, B, dtype=np.float64), w)
    print(f"fp64 model, mean interior endpoint error: {epe:.4f} px")
    assert epe <= 0.5


# ------------------------------------------------------------------------------------------------ 3. flags, symbols, argument checks
def test_fav_flow_usage_errors(favlib, tmp_path):
    assert os.path.exists(FLOW)
    r = _run([FLOW])
    assert r.returncode == 2 and "usage: fav_flow" in r.stderr
    r = _run([FLOW, "a.ppm", "b.ppm"])
    assert r.returncode == 2 and "expected <img1.ppm> <img2.ppm> <out.flo> [downscale]" in r.stderr
    r = _run([FLOW, "a.ppm", "b.ppm", "c.flo", "2", "extra"])
    assert r.returncode == 2 and "usage" in r.stderr
    r = _run([FLOW, "-frobnicate", "1", "a.ppm", "b.ppm", "c.flo"])
    assert r.returncode == 2 and "unknown option -frobnicate" in r.stderr
    r = _run([FLOW, "-iters", "many", "a.ppm", "b.ppm", "c.flo"])
    assert r.returncode == 2 and "bad value for -iters" in r.stderr
    r = _run([FLOW, "-iters", "5000", "a.ppm", "b.ppm", "c.flo"])          # the library's range check, before any file or device
    assert r.returncode == 1 and "iters must be" in r.stderr
    r = _run([FLOW, "-batch", "list.txt", "a.ppm"])
    assert r.returncode == 2 and "-batch takes its file names from the list" in r.stderr
    r = _run([FLOW, "-batch", str(tmp_path / "missing.txt")])
    assert r.returncode == 1 and "Could not open" in r.stderr
    (tmp_path / "bad.txt").write_text("a.ppm b.ppm\n")
    r = _run([FLOW, "-batch", str(tmp_path / "bad.txt")])
    assert r.returncode == 1 and 'bad.txt:1: expected "img1 img2 out.flo"' in r.stderr
    # four positional arguments are run-deepflow.sh's: accepted (the run then ends at the missing device or the missing file)
    r = _run([FLOW, str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm"), str(tmp_path / "c.flo"), "2"])
    # ("usage:", the message's first word: the temporary directory carries this test's name, and a missing file's path is printed)
    assert r.returncode == 1 and "usage:" not in r.stderr and ("no HIP device" in r.stderr or "Could not open" in r.stderr)
    assert not os.path.exists(tmp_path / "c.flo")


BASE = [STYLIZE, "-input_pattern", "v/f_%05d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/out"]


def test_fav_stylize_estimate_flow_flags(favlib):
    r = _run(BASE + ["-estimate_flow", "1", "-dry_run", "1"])                 # needs -input_pattern only
    assert r.returncode == 0 and "Must give" not in r.stderr, r.stderr
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["streams"][0]["flow_pattern"] == ""
    # ... and goes through the -streams / -gpus launcher unchanged
    r = _run([STYLIZE, "-input_pattern", "v/%S/f_%05d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/%S/out", "-estimate_flow", "1",
              "-flow_alpha", "12.5", "-flow_iters", "20", "-flow_warps", "2", "-flow_levels", "3", "-streams", "x,y,z", "-gpus", "2", "-dry_run", "1"])
    assert r.returncode == 0, r.stderr
    recs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{\"rank")), key=lambda d: d["rank"])
    assert [[s["name"] for s in d["streams"]] for d in recs] == [["x", "z"], ["y"]]
    for flag, pat in (("-flow_pattern", "v/bw_[%d]_{%d}.flo"), ("-forward_flow_pattern", "v/fw_{%d}_[%d].flo"), ("-occlusions_pattern", "v/r_[%d]_{%d}.pgm")):
        r = _run(BASE + ["-estimate_flow", "1", flag, pat, "-dry_run", "1"])
        assert r.returncode != 0 and "-estimate_flow 1" in r.stderr and f"cannot be combined with {flag}" in r.stderr, r.stderr
    r = _run(BASE + ["-estimate_flow", "1", "-scale_factor", "0.5", "-dry_run", "1"])
    assert r.returncode != 0 and "-estimate_flow 1 cannot be combined with a -scale_factor other than 1" in r.stderr
    for bad in ("2", "yes", ""):
        r = _run(BASE + ["-estimate_flow", bad, "-dry_run", "1"])
        assert r.returncode != 0 and "-estimate_flow must be 0 or 1" in r.stderr, (bad, r.stderr)
    r = _run(BASE + ["-estimate_flow", "1", "-flow_iters", "5000", "-dry_run", "1"])
    assert r.returncode != 0 and "iters must be" in r.stderr
    r = _run(BASE + ["-estimate_flow", "1", "-flow_alpha", "-3", "-dry_run", "1"])
    assert r.returncode != 0 and "alpha must be" in r.stderr
    # the flag is additive: without it the reference's message stands
    r = _run(BASE + ["-estimate_flow", "0", "-dry_run", "1"])
    assert r.returncode != 0 and "Must give -flow_pattern and -occlusions_pattern" in r.stderr
    r = _run(BASE + ["-estimate_flow", "1", "-gpu", "-1"])
    assert r.returncode != 0 and "no CPU backend" in r.stderr


def test_fav_stylize_vr_has_no_estimate_flow(favlib):
    r = _run([os.path.join(BIN, "fav_stylize_vr"), "-input_pattern", "v/f_%05d-%d.ppm", "-estimate_flow", "1", "-dry_run", "1"])
    assert r.returncode != 0 and "unknown option -estimate_flow" in r.stderr, r.stderr


def test_flow_exports_binding_and_argument_checks(favlib):
    out = subprocess.run(["nm", "-D", "--defined-only", favlib.LIB_PATH], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ("fav_flow_workspace_bytes", "fav_flow_rgb8", "fav_flow_grey_f32", "fav_flow_down_f32", "fav_flow_up_f32",
                 "fav_flow_coefficients_f32", "fav_flow_sweeps_f32", "fav_stream_next_frame_estimate"):
        assert name in defined and name in favlib.EXPORTS, name
    for fn in ("flow_rgb8", "flow_grey", "flow_down", "flow_up", "flow_coefficients", "flow_sweeps", "flow_workspace_bytes"):
        assert callable(getattr(favlib, fn))
    assert callable(favlib.Stream.next_frame_estimate)
    L = favlib.lib()
    # the workspace: every level's two grey images and two flows (level 0: one, the other is flow_out) + the coefficients, 256-byte sections
    sizes = M.level_sizes(720, 1280)
    r256 = lambda n: (n + 255) // 256 * 256
    want = sum(2 * r256(h * w * 4) + (2 if l else 1) * r256(h * w * 8) for l, (h, w) in enumerate(sizes)) + r256(720 * 1280 * 16)
    assert favlib.flow_workspace_bytes(1280, 720) == want
    assert favlib.flow_workspace_bytes(1280, 720, levels=1) < want
    # sizes below 16 x 16 and options out of range: 0 bytes / FAV_EINVAL with a message, device or not
    for w, h, opts, msg in ((15, 16, {}, "at least 16x16"), (16, 15, {}, "at least 16x16"), (64, 64, {"levels": 7}, "levels must be"),
                            (64, 64, {"warps": -1}, "warps must be"), (64, 64, {"iters": 1001}, "iters must be"),
                            (64, 64, {"alpha": -1.0}, "alpha must be"), (64, 64, {"alpha": float("nan")}, "alpha must be"),
                            (64, 64, {"sweeps_per_launch": 17}, "sweeps_per_launch must be")):
        o = favlib._flow_opts(opts)
        assert L.fav_flow_workspace_bytes(w, h, C.cast(C.pointer(o), C.c_void_p)) == 0 and msg.encode() in L.fav_last_error(), (w, h, opts)
        assert L.fav_flow_rgb8(C.c_void_p(256), C.c_void_p(256), w, h, C.byref(o), C.c_void_p(256), C.c_void_p(256), C.c_size_t(1 << 30), None) == -1
        assert msg.encode() in L.fav_last_error()
    assert L.fav_flow_rgb8(None, None, 64, 64, None, None, None, C.c_size_t(0), None) == -1 and b"null pointer" in L.fav_last_error()
    assert L.fav_flow_rgb8(C.c_void_p(256), C.c_void_p(256), 64, 64, None, C.c_void_p(256), C.c_void_p(256), C.c_size_t(16), None) == -1
    assert b"workspace holds 16 bytes" in L.fav_last_error()
    import torch
    if not torch.cuda.is_available():      # valid arguments, no device: FAV_ENODEVICE before anything is dereferenced
        nb = favlib.flow_workspace_bytes(64, 64)
        assert L.fav_flow_rgb8(C.c_void_p(256), C.c_void_p(256), 64, 64, None, C.c_void_p(256), C.c_void_p(256), C.c_size_t(nb), None) == -6
        assert b"no CPU fallback" in L.fav_last_error()
        assert L.fav_flow_grey_f32(C.c_void_p(256), C.c_void_p(256), 64, 64, None) == -6
