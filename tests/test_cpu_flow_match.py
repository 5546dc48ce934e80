"""Host side of the estimator's block-matching prior (fav_flow_opts_ex2.match_beta; no GPU needed): the premise that it recovers objects
which move further than their own size, what it costs where nothing moves far, the algebra of the tensor with the prior off, the ABI of the
_ex2 entries, the flags of the three executables and the resource report of the new kernels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402
import flow_grad_model as G  # noqa: E402
import flow_match_model as P  # noqa: E402
from flow_testing import kernel_resource_usage  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fast-artistic-videos_amd")
BIN = os.path.join(PKG, "bin")
FLOW, STYLIZE, STYLIZE_VR = (os.path.join(BIN, n) for n in ("fav_flow", "fav_stylize", "fav_stylize_vr"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LEVELS = 4          # the premise's pyramid at 192 x 256
MARGIN = 0.2        # px: what the prior may cost where nothing moves far (measured: 0.12 and 0.13 px; the matches are integers at half
#                     resolution, i.e. a pull towards a displacement that is up to 1 px off at full size)


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=60)


# ------------------------------------------------------------------------------------------------ 1. the premise
@pytest.mark.parametrize("seed,rect,fg,bg", P.LARGE)
def test_prior_recovers_an_object_that_outruns_the_pyramid(seed, rect, fg, bg):
    """192 x 256, 4 levels, fp64 models, mean endpoint error in px (12 px of frame border excluded) on the object / on the non-occluded
    background.  Measured, plain estimator (alpha 15) -> with the prior (beta 225, R 16):
      seed 1, 24 x 24 moving (22, -14):  22.40 / 0.151 -> 4.72 / 0.195
      seed 2, 30 x 30 moving (-26, 9):   35.11 / 0.209 -> 4.49 / 0.491
      seed 3, 48 x 48 moving (30, 20):   35.05 / 0.322 -> 3.24 / 0.608
    Required: object <= 0.25 x plain, background <= plain + 0.5 px."""
    A, B, truth, valid, obj = P.scene(P.SCENE_H, P.SCENE_W, seed, rect, fg, bg)
    plain = P.scene_errors(M.flow(A, B, levels=LEVELS, dtype=np.float64), truth, valid, obj)
    prior = P.scene_errors(P.flow(A, B, levels=LEVELS, dtype=np.float64), truth, valid, obj)
    print(f"seed {seed} {rect} fg {fg}: plain {plain[0]:.3f} / {plain[1]:.3f} px, prior {prior[0]:.3f} / {prior[1]:.3f} px")
    assert prior[0] <= 0.25 * plain[0] and prior[1] <= plain[1] + 0.5


def test_prior_costs_little_where_nothing_moves_far():
    """the small-motion scene (fg (-3, 1.5) over bg (2, 0)) and the constant shift shifted_pair(1, 192, 256).  Measured, plain -> prior:
    scene 0.463 / 0.528 -> 0.582 / 0.478 px; shifted pair 0.0434 -> 0.1754 px (0.1244 at beta 25).  Required: <= plain + 0.2 px, each."""
    seed, rect, fg, bg = P.SMALL
    A, B, truth, valid, obj = P.scene(P.SCENE_H, P.SCENE_W, seed, rect, fg, bg)
    plain = P.scene_errors(M.flow(A, B, levels=LEVELS, dtype=np.float64), truth, valid, obj)
    prior = P.scene_errors(P.flow(A, B, levels=LEVELS, dtype=np.float64), truth, valid, obj)
    print(f"small motion: plain {plain[0]:.3f} / {plain[1]:.3f} px, prior {prior[0]:.3f} / {prior[1]:.3f} px")
    assert prior[0] <= plain[0] + MARGIN and prior[1] <= plain[1] + MARGIN
    A, B, t = M.shifted_pair(1, P.SCENE_H, P.SCENE_W)
    plain = M.interior_epe(M.flow(A, B, levels=LEVELS, dtype=np.float64), t)
    prior = M.interior_epe(P.flow(A, B, levels=LEVELS, dtype=np.float64), t)
    print(f"shifted pair: plain {plain:.4f} px, prior {prior:.4f} px")
    assert prior <= plain + MARGIN


# ------------------------------------------------------------------------------------------------ 2. the model's own algebra
def test_tensor_with_bm_zero_is_the_old_sweep():
    """m == 0 everywhere (and, separately, a gate that is never on): the brightness tensor's five stored values and the tensor sweep must
    give flow_model.sweeps back, in fp64 to 1e-12"""
    A, B = M.warped_pair(64, 64, 11)
    gA, gB = M.grey(A, np.float64), M.grey(B, np.float64)
    f0 = np.random.default_rng(3).standard_normal((64, 64, 2))
    coef = M.coefficients(gA, gB, f0, M.ALPHA, np.float64)
    d = np.random.default_rng(4).integers(-16, 17, (64, 64, 2)).astype(np.float64)
    for m, tau in ((np.zeros((64, 64)), 1.0), (np.ones((64, 64)), 1e9)):
        q = P.coefficients(gA, gB, f0, d, m, M.ALPHA, 225.0, tau, dtype=np.float64)
        for n in (1, 30):
            want = M.sweeps(f0, coef, n, np.float64)
            assert np.abs(G.sweeps(f0, q, n, np.float64) - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (n, tau)
    # ... and with the gate on it is another estimator
    q = P.coefficients(gA, gB, f0, d, np.ones((64, 64)), M.ALPHA, 225.0, 1.0, dtype=np.float64)
    assert np.abs(G.sweeps(f0, q, 30, np.float64) - M.sweeps(f0, coef, 30, np.float64)).max() > 1.0


def test_match_model_on_a_known_shift_and_its_tie_rule():
    from fav_amd import synth
    g = M.grey(synth.smooth_frame(40, 52, 3), np.float64)
    b = np.roll(g, (3, -5), (0, 1))          # B(q + (-5, 3)) = A(q) away from the wrap
    d_ab, d_ba = P.match(g, b, 8), P.match(b, g, 8)
    assert (d_ab[12:28, 14:38] == (-5, 3)).all() and (d_ba[12:28, 14:38] == (5, -3)).all()
    m = P.check(d_ab, d_ba)
    assert m[12:25, 19:38].all() and set(np.unique(m)) <= {0.0, 1.0}
    # two constant planes: every cost is equal, so the first displacement in the order wins
    flat = np.full((9, 11), 7.0)
    assert (P.match(flat, flat, 2) == (-2, -2)).all()
    # the prior's pyramid: sizes, m in [0, 1], fp32 stays fp32
    sizes = M.level_sizes(80, 104, 3)
    full = np.zeros(sizes[1] + (2,), np.int64); full[..., 0] = 4
    pyr = P.prior_pyramid(full, np.ones(sizes[1]), sizes)
    for (dl, ml), (h, w) in zip(pyr, sizes):
        assert dl.shape == (h, w, 2) and ml.shape == (h, w) and dl.dtype == np.float32 and ml.min() >= 0 and ml.max() <= 1
    assert np.allclose(pyr[0][0][..., 0], 8.0) and np.allclose(pyr[2][0][..., 0], 2.0) and (pyr[0][0][..., 1] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the ABI
EX2_ENTRIES = ("fav_flow_workspace_bytes_ex2", "fav_flow_rgb8_ex2", "fav_flow_pairs_workspace_bytes_ex2", "fav_flow_pairs_rgb8_ex2",
               "fav_stream_next_frame_estimate_ex2", "fav_flow_match_f32", "fav_flow_match_check", "fav_flow_coefficients_prior_f32")


def _r256(n):
    return (n + 255) // 256 * 256


def test_ex2_entries_struct_sizes_and_workspace(favlib):
    L = favlib.lib()
    assert C.sizeof(favlib._FlowOpts) == 24 and C.sizeof(favlib._FlowOptsEx) == 28 and C.sizeof(favlib._FlowOptsEx2) == 36
    hdr = open(os.path.join(ROOT, "include", "fav.h")).read()
    assert "typedef struct fav_flow_opts_ex2 { fav_flow_opts_ex ex; float match_beta; int match_radius; } fav_flow_opts_ex2;" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", favlib.LIB_PATH], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EX2_ENTRIES:
        assert name in defined and name in favlib.EXPORTS and name + "(" in hdr and name in integration, name
    assert callable(favlib.flow_match) and callable(favlib.flow_match_check) and callable(favlib.flow_coefficients_prior)
    void = lambda o: C.cast(C.pointer(o), C.c_void_p)
    for (w, h) in ((1280, 720), (64, 64), (150, 203)):
        for opts in ({}, dict(smooth_eps=0.3), dict(data_term=1), dict(data_term=1, smooth_eps=0.3)):
            ex = favlib._flow_opts_ex(opts)
            off = favlib._flow_opts_ex2(dict(opts, match_beta=0.0, match_radius=7))
            old = L.fav_flow_workspace_bytes_ex(w, h, void(ex))
            assert old > 0 and L.fav_flow_workspace_bytes_ex2(w, h, void(off)) == old == favlib.flow_workspace_bytes(w, h, **opts)
            if not opts:
                assert L.fav_flow_workspace_bytes_ex2(w, h, None) == old == L.fav_flow_workspace_bytes(w, h, None)
            for n in (1, 6):
                assert L.fav_flow_pairs_workspace_bytes_ex2(w, h, n, void(off)) == L.fav_flow_pairs_workspace_bytes_ex(w, h, n, void(ex)) > 0
            # the option on: per match field 4 bytes per level-1 pixel (a single flow: two fields), per flow 12 bytes per pixel of the
            # levels >= 1 and, with the brightness term, 20 instead of 16 bytes of coefficients
            sizes = M.level_sizes(h, w)
            prior = sum(_r256(hh * ww * 12) for hh, ww in sizes[1:])
            field = _r256(sizes[1][0] * sizes[1][1] * 4)
            coef = 0 if opts.get("data_term") else _r256(w * h * 20) - _r256(w * h * 16)
            assert favlib.flow_workspace_bytes(w, h, match_beta=-1, **opts) == old + 2 * field + prior + coef
            assert favlib.flow_workspace_bytes(w, h, match_beta=225.0, match_radius=32, **opts) == old + 2 * field + prior + coef
            for n in (1, 6):
                assert favlib.flow_pairs_workspace_bytes(w, h, n, match_beta=-1, **opts) == \
                    favlib.flow_pairs_workspace_bytes(w, h, n, **opts) + 2 * n * (field + prior + coef)


def test_bad_match_options_are_refused_before_the_device(favlib):
    L = favlib.lib()
    void = lambda o: C.cast(C.pointer(o), C.c_void_p)
    one = (C.c_void_p * 1)(256)
    p = C.c_void_p(256)
    bad = [(dict(match_beta=2e6), b"match_beta must be"), (dict(match_beta=float("nan")), b"match_beta must be"), (dict(match_beta=float("inf")), b"match_beta must be"),
           (dict(match_beta=-1, match_radius=33), b"match_radius must be"), (dict(match_beta=-1, match_radius=-1), b"match_radius must be"),
           (dict(match_radius=40), b"match_radius must be"), (dict(match_beta=-1, levels=1), b"at least two levels")]
    for opts, msg in bad:
        o = favlib._flow_opts_ex2(opts)
        assert L.fav_flow_workspace_bytes_ex2(64, 64, void(o)) == 0 and msg in L.fav_last_error(), opts
        assert L.fav_flow_pairs_workspace_bytes_ex2(64, 64, 2, void(o)) == 0 and msg in L.fav_last_error(), opts
        assert L.fav_flow_rgb8_ex2(p, p, 64, 64, C.byref(o), p, p, C.c_size_t(1 << 30), None) == -1 and msg in L.fav_last_error(), opts      # FAV_EINVAL
        assert L.fav_flow_pairs_rgb8_ex2(one, one, 1, 64, 64, C.byref(o), one, one, p, C.c_size_t(1 << 30), None) == -1 and msg in L.fav_last_error(), opts
        with pytest.raises(favlib.FavError):
            favlib.flow_workspace_bytes(64, 64, **opts)
    # a frame too small for a second level: 16 x 16 .. 31 x 31 have one
    o = favlib._flow_opts_ex2(dict(match_beta=-1))
    assert L.fav_flow_workspace_bytes_ex2(24, 24, void(o)) == 0 and b"at least two levels" in L.fav_last_error()
    assert L.fav_flow_workspace_bytes_ex2(24, 24, void(favlib._flow_opts_ex2({}))) > 0
    # the other options are still checked through the _ex2 entries
    assert L.fav_flow_workspace_bytes_ex2(64, 64, void(favlib._flow_opts_ex2(dict(match_beta=-1, data_term=2)))) == 0 and b"data_term must be" in L.fav_last_error()
    with pytest.raises(favlib.FavError, match="unknown flow option"):
        favlib.flow_workspace_bytes(64, 64, match_betas=1)
    # the stage entries' own checks
    f = C.c_float
    q = C.c_void_p(512)
    for r in (0, 33, -1):
        assert L.fav_flow_match_f32(p, p, 64, 64, r, p, q, None) == -1 and b"radius must be 1 .. 32" in L.fav_last_error(), r
    assert L.fav_flow_match_f32(p, p, 64, 64, 16, p, p, None) == -1 and b"bad argument" in L.fav_last_error()
    assert L.fav_flow_match_f32(None, p, 64, 64, 16, p, q, None) == -1 and L.fav_flow_match_check(p, None, 64, 64, p, None) == -1
    assert L.fav_flow_match_check(C.c_void_p(258), p, 64, 64, p, None) == -1 and b"4-byte aligned" in L.fav_last_error()
    coef = lambda beta, tau, term, wp, hp: L.fav_flow_coefficients_prior_f32(p, p, p, f(15.0), f(0.0), term, p, wp, hp, f(beta), f(tau), q, None, 64, 64, None)
    for beta in (0.0, -1.0, 2e6, float("nan")):
        assert coef(beta, 1.0, 0, 64, 64) == -1 and b"beta must be" in L.fav_last_error(), beta
    assert coef(225.0, -1.0, 0, 64, 64) == -1 and b"tau must be" in L.fav_last_error()
    assert coef(225.0, 1.0, 2, 64, 64) == -1 and b"data_term must be" in L.fav_last_error()
    assert coef(225.0, 1.0, 0, 31, 32) == -1 and b"the prior must have" in L.fav_last_error()
    import torch
    if not torch.cuda.is_available():      # valid arguments, no device: FAV_ENODEVICE before anything is dereferenced
        o = favlib._flow_opts_ex2(dict(match_beta=-1))
        nb = favlib.flow_workspace_bytes(64, 64, match_beta=-1)
        assert L.fav_flow_rgb8_ex2(p, p, 64, 64, C.byref(o), p, p, C.c_size_t(nb), None) == -6
        assert L.fav_flow_rgb8_ex2(p, p, 64, 64, C.byref(o), p, p, C.c_size_t(nb - 1), None) == -1
        assert L.fav_flow_match_f32(p, p, 64, 64, 16, p, q, None) == -6 and L.fav_flow_match_check(p, q, 64, 64, p, None) == -6
        assert coef(225.0, 1.0, 1, 32, 32) == -6 and coef(225.0, 1.0, 0, 64, 64) == -6


# ------------------------------------------------------------------------------------------------ 4. the flags
def test_fav_flow_match_flags(favlib, tmp_path):
    r = _run([FLOW])
    assert r.returncode == 2 and "[-match 0|1] [-match_radius n]" in r.stderr
    for bad in ("2", "yes", "-1"):
        r = _run([FLOW, "-match", bad, "a.ppm", "b.ppm", "c.flo"])
        assert r.returncode == 2 and "-match must be 0 or 1" in r.stderr, (bad, r.stderr)
    r = _run([FLOW, "-match", "1", "-match_radius", "40", "a.ppm", "b.ppm", "c.flo"])
    assert r.returncode == 1 and "match_radius must be" in r.stderr, r.stderr
    r = _run([FLOW, "-match", "1", "-levels", "1", "a.ppm", "b.ppm", "c.flo"])
    assert r.returncode == 1 and "at least two levels" in r.stderr, r.stderr
    r = _run([FLOW, "-match", "1", "-match_radius", "8", "-grad", "1", "-eps", "0.3", str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm"), str(tmp_path / "c.flo")])
    assert r.returncode == 1 and "usage" not in r.stderr and ("no HIP device" in r.stderr or "Could not open" in r.stderr)      # accepted


def test_fav_stylize_flow_match_flag(favlib):
    base = [STYLIZE, "-input_pattern", "v/f_%05d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/out"]
    r = _run(base + ["-estimate_flow", "1", "-flow_match", "1", "-flow_grad", "1", "-flow_eps", "0.3", "-dry_run", "1"])
    assert r.returncode == 0, r.stderr
    r = _run(base + ["-estimate_flow", "1", "-flow_match", "0", "-dry_run", "1"])
    assert r.returncode == 0, r.stderr
    r = _run(base + ["-flow_pattern", "v/b_%05d.flo", "-occlusions_pattern", "v/r_%05d.pgm", "-flow_match", "1", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_match" in r.stderr and "-estimate_flow 1" in r.stderr, r.stderr
    r = _run(base + ["-estimate_flow", "1", "-flow_match", "2", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_match must be 0 or 1" in r.stderr, r.stderr
    r = _run(base + ["-estimate_flow", "1", "-flow_match", "1", "-flow_levels", "1", "-dry_run", "1"])
    assert r.returncode != 0 and "at least two levels" in r.stderr, r.stderr


def test_fav_stylize_vr_flow_match_flag(favlib):
    equi = [STYLIZE_VR, "-input_equi_pattern", "v/e_%05d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/out"]
    ok = _run(equi + ["-dry_run", "1"])
    r = _run(equi + ["-flow_match", "1", "-flow_grad", "1", "-flow_eps", "0.3", "-dry_run", "1"])
    assert r.returncode == ok.returncode and "unknown option" not in r.stderr and "-flow_match" not in r.stderr, r.stderr
    faces = [STYLIZE_VR, "-input_pattern", "v/f_%05d-%d.ppm", "-flow_pattern", "v/b_%05d-%d.flo", "-occlusions_pattern", "v/r_%05d-%d.pgm", "-model_vid", "m.t7",
             "-output_prefix", "o/out"]
    r = _run(faces + ["-flow_match", "1", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_match" in r.stderr and "-input_equi_pattern" in r.stderr, r.stderr
    r = _run(equi + ["-flow_match", "3", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_match must be 0 or 1" in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ 5. the resource gate
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_matching_prior_kernels_do_not_spill(tmp_path):
    """the compiler's kernel-resource-usage remarks for kernels_flow.hip (flow_testing.kernel_resource_usage).  flow_match_kernel keeps 28
    packed words of A, 14 row sums and 8 running minima per lane in registers: scratch 0, at least two waves per SIMD, and an LDS tile
    (the A tile and the B search window for the largest radius) of which several fit a CU.  Measured: 96 VGPRs, occupancy 5, LDS
    17 560 B; flow_coef_prior_kernel 61 | 57 (weights) | 53 (gradients) | 77 (both) VGPRs; the two small kernels 10 and 34."""
    usage = kernel_resource_usage(HIPCC, tmp_path)
    match = [u for k, u in usage.items() if "flow_match_kernel" in k]
    small = {k: u for k, u in usage.items() if "flow_match_check_kernel" in k or "flow_prior_down_kernel" in k}
    coefs = {k: u for k, u in usage.items() if "flow_coef_prior_kernel" in k}
    assert len(match) == 1 and len(small) == 2 and len(coefs) == 4, sorted(usage)
    print("flow_match_kernel", match[0])
    assert match[0]["ScratchSize"] == 0 and match[0]["AGPRs"] == 0 and match[0]["Occupancy"] >= 2 and 0 < match[0]["LDS"] <= 32768, match
    for k, u in {**small, **coefs}.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["Occupancy"] >= 2 and u["LDS"] == 0, (k, u)
    # the prior adds no sweep kernel: the four instantiations of before
    assert len([k for k in usage if "flow_sweep_kernel" in k]) == 4
