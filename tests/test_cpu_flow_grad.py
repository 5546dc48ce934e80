"""Host side of the estimator's gradient-constancy data term (fav_flow_opts_ex.data_term = FAV_FLOW_DATA_GRADIENT; no GPU needed): the
premise that it survives a change of lighting that the brightness term reads as motion, the algebra of the stored form, the ABI of the
_ex entries, the flags of the three executables and the resource report of the new kernels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402
import flow_robust_model as R  # noqa: E402
import flow_grad_model as G  # noqa: E402
from flow_testing import kernel_resource_usage  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fast-artistic-videos_amd")
BIN = os.path.join(PKG, "bin")
FLOW, STYLIZE, STYLIZE_VR = (os.path.join(BIN, n) for n in ("fav_flow", "fav_stylize", "fav_stylize_vr"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=60)


# ------------------------------------------------------------------------------------------------ 1. the premise
_pairs = {}


def _pair(seed, h, w):
    """(A, B, truth, brightness error, gradient error) of an unrelit pair, computed once"""
    if (seed, h, w) not in _pairs:
        A, B, t = M.shifted_pair(seed, h, w)
        _pairs[(seed, h, w)] = (A, B, t, M.interior_epe(M.flow(A, B, dtype=np.float64), t), M.interior_epe(G.flow(A, B, alpha=8.0, dtype=np.float64), t))
    return _pairs[(seed, h, w)]


@pytest.mark.parametrize("gain,offset", G.RELIGHTS)
@pytest.mark.parametrize("seed,h,w", G.PAIRS)
def test_gradient_term_survives_relighting(seed, h, w, gain, offset):
    """flow_model.shifted_pair, true flow (+3.5, -2.25) px, B relit as clip(rint(gain B + offset)); fp64 models, default options, alpha 8
    for the gradient term; mean interior endpoint error in px.  Measured, brightness -> gradients:
      seed 1  96x128: 0.8 B + 10  6.69 -> 0.280;  0.7 B  19.05 -> 0.431;  B + 25   9.00 -> 0.188
      seed 2  96x128: 0.8 B + 10  6.48 -> 0.249;  0.7 B  13.54 -> 0.417;  B + 25  11.60 -> 0.131
      seed 1 150x203: 0.8 B + 10  4.57 -> 0.266;  0.7 B  17.18 -> 0.430;  B + 25  10.72 -> 0.112
    Required: gradients <= 0.6 px and <= 0.1 x brightness on the same relit pair."""
    A, B, t = _pair(seed, h, w)[:3]
    Br = G.relight(B, gain, offset)
    bright = M.interior_epe(M.flow(A, Br, dtype=np.float64), t)
    grad = M.interior_epe(G.flow(A, Br, alpha=8.0, dtype=np.float64), t)
    print(f"seed {seed} {h}x{w}, {gain} B + {offset}: brightness {bright:.3f} px, gradients {grad:.3f} px, ratio {grad / bright:.3f}")
    assert grad <= 0.6 and grad <= 0.1 * bright


@pytest.mark.parametrize("seed,h,w", G.PAIRS)
def test_gradient_term_in_constant_light(seed, h, w):
    """the same pairs unrelit.  Measured, brightness -> gradients: 0.066 -> 0.110, 0.098 -> 0.130, 0.038 -> 0.080 px.  Required: <= 0.2 px"""
    _, _, _, bright, grad = _pair(seed, h, w)
    print(f"seed {seed} {h}x{w}, same light: brightness {bright:.3f} px, gradients {grad:.3f} px")
    assert grad <= 0.2


@pytest.mark.parametrize("h,w,seed", [(96, 128, 1), (96, 128, 2)])
def test_gradient_term_with_edge_preserving_smoothness_survives_relighting(h, w, seed):
    """flow_robust_model.two_motion_scene relit 0.8 B + 10, smooth_eps 0.3, the default alpha of the combination (8: DESIGN.md has the
    table it was chosen from).  Measured, robust brightness model -> gradient model: seed 1 10.84 -> 1.52 px; seed 2 8.37 -> 1.57 px.
    Required: gradients <= 0.5 x brightness."""
    A, B, truth, valid = R.two_motion_scene(h, w, seed)
    Br = G.relight(B, 0.8, 10.0)
    bright = R.scene_epe(R.flow(A, Br, eps=0.3, dtype=np.float64), truth, valid)
    grad = R.scene_epe(G.flow(A, Br, eps=0.3, dtype=np.float64), truth, valid)
    print(f"two motions {h}x{w} seed {seed}, 0.8 B + 10, eps 0.3: brightness {bright:.3f} px, gradients {grad:.3f} px, ratio {grad / bright:.3f}")
    assert G.ALPHA_ROBUST == 8.0 and grad <= 0.5 * bright


# ------------------------------------------------------------------------------------------------ 2. the algebra of the stored form
def test_tensor_sweep_of_one_channel_is_the_old_sweep():
    """a tensor built from ONE channel (a, b, c) of flow_model.coefficients -- J = [[a^2, a b], [a b, b^2]], h = (a c, b c) -- with
    w = alpha^2: the five stored values and the tensor sweep must give flow_model.sweeps back, in fp64 to 1e-12"""
    A, B = M.warped_pair(64, 64, 11)
    gA, gB = M.grey(A, np.float64), M.grey(B, np.float64)
    f0 = np.random.default_rng(3).standard_normal((64, 64, 2))
    coef = M.coefficients(gA, gB, f0, M.ALPHA, np.float64)
    a, b, c = coef[..., 0], coef[..., 1], coef[..., 2]
    q = G.stored_form(a * a, a * b, b * b, a * c, b * c, np.float64(M.ALPHA) * np.float64(M.ALPHA))
    for n in (1, 30):
        want = M.sweeps(f0, coef, n, np.float64)
        got = G.sweeps(f0, q, n, np.float64)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), n
    # ... and with the weighted mean, against flow_robust_model.sweeps
    rc, wt = R.coefficients(gA, gB, f0, 5.0, 0.3, np.float64)
    _, S = R.edge_weights(R.diffusivity(f0, 0.3, np.float64), np.float64)
    a, b, c = rc[..., 0], rc[..., 1], rc[..., 2]
    q = G.stored_form(a * a, a * b, b * b, a * c, b * c, (25.0 * S) * 0.25)
    want = R.sweeps(f0, rc, wt, 30, np.float64)
    assert np.abs(G.sweeps(f0, q, 30, np.float64, wt) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_model_sweeps_compose_and_fp32_stays_fp32():
    from fav_amd import synth
    f0 = np.random.default_rng(5).standard_normal((19, 27, 2)).astype(np.float32)
    A, B = M.grey(synth.smooth_frame(19, 27, 1)), M.grey(synth.smooth_frame(19, 27, 2))
    for eps in (0.0, 0.3):
        coef, wt = G.coefficients(A, B, f0, 8.0, eps) if eps else (G.coefficients(A, B, f0, 8.0), None)
        assert coef.shape == (19, 27, 5) and coef.dtype == np.float32 and np.isfinite(coef).all()
        step = f0
        for _ in range(7):
            step = G.sweeps(step, coef, 1, weights=wt)
        assert np.array_equal(G.sweeps(f0, coef, 7, weights=wt), step)


# ------------------------------------------------------------------------------------------------ 3. the ABI
EX_ENTRIES = ("fav_flow_workspace_bytes_ex", "fav_flow_rgb8_ex", "fav_flow_pairs_workspace_bytes_ex", "fav_flow_pairs_rgb8_ex",
              "fav_stream_next_frame_estimate_ex", "fav_flow_coefficients_grad_f32", "fav_flow_sweeps_grad_f32")


def _r256(n):
    return (n + 255) // 256 * 256


def test_ex_entries_and_struct_sizes(favlib):
    L = favlib.lib()
    assert C.sizeof(favlib._FlowOpts) == 24 and C.sizeof(favlib._FlowOptsEx) == 28
    hdr = open(os.path.join(ROOT, "include", "fav.h")).read()
    assert "typedef struct fav_flow_opts_ex { fav_flow_opts base; int data_term; } fav_flow_opts_ex;" in hdr
    assert "#define FAV_FLOW_DATA_GRADIENT 1" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", favlib.LIB_PATH], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in EX_ENTRIES:
        assert name in defined and name in favlib.EXPORTS and name + "(" in hdr, name
    assert callable(favlib.flow_coefficients_grad) and callable(favlib.flow_sweeps_grad)
    void = lambda o: C.cast(C.pointer(o), C.c_void_p)
    for (w, h, want) in ((1280, 720, 36858368), (64, 64, None)):
        old = L.fav_flow_workspace_bytes(w, h, None)
        assert old > 0 and (want is None or old == want)
        assert L.fav_flow_workspace_bytes_ex(w, h, None) == old
        assert L.fav_flow_workspace_bytes_ex(w, h, void(favlib._flow_opts_ex({}))) == old
        assert favlib.flow_workspace_bytes(w, h) == favlib.flow_workspace_bytes(w, h, data_term=0) == favlib.flow_workspace_bytes(w, h, gradient_data=False) == old
        # the option on: 20 instead of 16 bytes of coefficients per pixel and flow, nothing else moves
        grown = _r256(w * h * 20) - _r256(w * h * 16)
        assert favlib.flow_workspace_bytes(w, h, data_term=1) == favlib.flow_workspace_bytes(w, h, gradient_data=True) == old + grown
        assert favlib.flow_workspace_bytes(w, h, data_term=1, smooth_eps=0.3) == favlib.flow_workspace_bytes(w, h, smooth_eps=0.3) + grown
        for n in (1, 6):
            assert L.fav_flow_pairs_workspace_bytes_ex(w, h, n, void(favlib._flow_opts_ex({}))) == L.fav_flow_pairs_workspace_bytes(w, h, n, None)
            assert favlib.flow_pairs_workspace_bytes(w, h, n, data_term=1) == favlib.flow_pairs_workspace_bytes(w, h, n) + 2 * n * grown


def test_bad_data_term_is_refused_before_the_device(favlib):
    L = favlib.lib()
    void = lambda o: C.cast(C.pointer(o), C.c_void_p)
    for bad in (2, -1, 7):
        o = favlib._flow_opts_ex({"data_term": bad})
        assert L.fav_flow_workspace_bytes_ex(64, 64, void(o)) == 0 and b"data_term must be" in L.fav_last_error(), bad
        assert L.fav_flow_pairs_workspace_bytes_ex(64, 64, 2, void(o)) == 0 and b"data_term must be" in L.fav_last_error(), bad
        assert L.fav_flow_rgb8_ex(C.c_void_p(256), C.c_void_p(256), 64, 64, C.byref(o), C.c_void_p(256), C.c_void_p(256), C.c_size_t(1 << 30), None) == -1      # FAV_EINVAL
        assert b"data_term must be" in L.fav_last_error()
        one = (C.c_void_p * 1)(256)
        assert L.fav_flow_pairs_rgb8_ex(one, one, 1, 64, 64, C.byref(o), one, one, C.c_void_p(256), C.c_size_t(1 << 30), None) == -1
        assert b"data_term must be" in L.fav_last_error()
        with pytest.raises(favlib.FavError, match="data_term must be"):
            favlib.flow_workspace_bytes(64, 64, data_term=bad)
    with pytest.raises(favlib.FavError, match="contradict"):
        favlib.flow_workspace_bytes(64, 64, data_term=0, gradient_data=True)
    with pytest.raises(favlib.FavError, match="unknown flow option"):
        favlib.flow_workspace_bytes(64, 64, data_terms=1)
    # the other options are still checked through the _ex entries
    o = favlib._flow_opts_ex({"data_term": 1, "smooth_eps": -0.3})
    assert L.fav_flow_workspace_bytes_ex(64, 64, void(o)) == 0 and b"smooth_eps must be" in L.fav_last_error()
    # the stage entries' own checks
    f = C.c_float
    assert L.fav_flow_coefficients_grad_f32(None, None, None, f(8.0), f(0.0), None, None, 64, 64, None) == -1 and b"bad argument" in L.fav_last_error()
    assert L.fav_flow_coefficients_grad_f32(C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), f(8.0), f(-1.0), C.c_void_p(256), C.c_void_p(512), 64, 64, None) == -1
    assert b"smooth_eps must be" in L.fav_last_error()
    assert L.fav_flow_coefficients_grad_f32(C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), f(8.0), f(0.3), C.c_void_p(256), C.c_void_p(264), 64, 64, None) == -1
    assert b"16-byte aligned" in L.fav_last_error()
    assert L.fav_flow_sweeps_grad_f32(C.c_void_p(256), C.c_void_p(256), None, 3, 17, C.c_void_p(256), C.c_void_p(256), 64, 64, None) == -1
    assert b"sweeps_per_launch 0 (default) .. 16" in L.fav_last_error()
    import torch
    if not torch.cuda.is_available():      # valid arguments, no device: FAV_ENODEVICE before anything is dereferenced
        o = favlib._flow_opts_ex({"data_term": 1})
        nb = favlib.flow_workspace_bytes(64, 64, data_term=1)
        assert L.fav_flow_rgb8_ex(C.c_void_p(256), C.c_void_p(256), 64, 64, C.byref(o), C.c_void_p(256), C.c_void_p(256), C.c_size_t(nb), None) == -6
        assert L.fav_flow_rgb8_ex(C.c_void_p(256), C.c_void_p(256), 64, 64, C.byref(o), C.c_void_p(256), C.c_void_p(256), C.c_size_t(nb - 1), None) == -1
        assert L.fav_flow_sweeps_grad_f32(C.c_void_p(256), C.c_void_p(256), None, 3, 0, C.c_void_p(256), C.c_void_p(256), 64, 64, None) == -6


# ------------------------------------------------------------------------------------------------ 4. the flags
def test_fav_flow_grad_flag(favlib, tmp_path):
    r = _run([FLOW])
    assert r.returncode == 2 and "[-grad 0|1]" in r.stderr
    for bad in ("2", "yes", "-1"):
        r = _run([FLOW, "-grad", bad, "a.ppm", "b.ppm", "c.flo"])
        assert r.returncode == 2 and "-grad must be 0 or 1" in r.stderr, (bad, r.stderr)
    r = _run([FLOW, "-grad", "1", "-eps", "0.3", str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm"), str(tmp_path / "c.flo")])      # accepted
    assert r.returncode == 1 and "usage" not in r.stderr and ("no HIP device" in r.stderr or "Could not open" in r.stderr)


def test_fav_stylize_flow_grad_flag(favlib):
    base = [STYLIZE, "-input_pattern", "v/f_%05d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/out"]
    r = _run(base + ["-estimate_flow", "1", "-flow_grad", "1", "-flow_eps", "0.3", "-dry_run", "1"])
    assert r.returncode == 0, r.stderr
    r = _run(base + ["-estimate_flow", "1", "-flow_grad", "0", "-dry_run", "1"])
    assert r.returncode == 0, r.stderr
    # outside -estimate_flow 1 the flag has nothing to select
    r = _run(base + ["-flow_pattern", "v/b_%05d.flo", "-occlusions_pattern", "v/r_%05d.pgm", "-flow_grad", "1", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_grad" in r.stderr and "-estimate_flow 1" in r.stderr, r.stderr
    r = _run(base + ["-estimate_flow", "1", "-flow_grad", "2", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_grad must be 0 or 1" in r.stderr, r.stderr


def test_fav_stylize_vr_flow_grad_flag(favlib):
    equi = [STYLIZE_VR, "-input_equi_pattern", "v/e_%05d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/out"]
    ok = _run(equi + ["-dry_run", "1"])
    r = _run(equi + ["-flow_grad", "1", "-dry_run", "1"])
    assert r.returncode == ok.returncode and "unknown option" not in r.stderr and "-flow_grad" not in r.stderr, r.stderr
    faces = [STYLIZE_VR, "-input_pattern", "v/f_%05d-%d.ppm", "-flow_pattern", "v/b_%05d-%d.flo", "-occlusions_pattern", "v/r_%05d-%d.pgm", "-model_vid", "m.t7",
             "-output_prefix", "o/out"]
    r = _run(faces + ["-flow_grad", "1", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_grad" in r.stderr and "-input_equi_pattern" in r.stderr, r.stderr
    r = _run(equi + ["-flow_grad", "3", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_grad must be 0 or 1" in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ 5. the resource gate
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_gradient_term_kernels_do_not_spill(tmp_path):
    """the compiler's kernel-resource-usage remarks for kernels_flow.hip (flow_testing.kernel_resource_usage): the two tensor sweeps
    keep five (nine with the edge weights) values per cell in registers -- scratch 0 -- at two waves per SIMD or better with the 32 KB
    LDS tile, and the two coefficient kernels do not spill either.  Measured: sweeps 128 VGPRs, occupancy 4 (plain mean) and 176 VGPRs,
    occupancy 2 (weighted mean); coefficients 53 VGPRs, occupancy 8 and 78 VGPRs, occupancy 6."""
    usage = kernel_resource_usage(HIPCC, tmp_path)
    sweeps = {k: u for k, u in usage.items() if "flow_sweep_kernel" in k and "GradCell" in k}
    coefs = {k: u for k, u in usage.items() if "flow_coef_grad_kernel" in k}
    assert len(sweeps) == 2 and len(coefs) == 2, sorted(usage)
    for k, u in {**sweeps, **coefs}.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["Occupancy"] >= 2, (k, u)
    for k, u in sweeps.items():
        assert u["LDS"] == 32768 and u["VGPRs"] + u["AGPRs"] <= 256, (k, u)
