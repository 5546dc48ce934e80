"""The estimator's edge-preserving smoothness (fav_flow_opts.smooth_eps > 0) on the GPU against its numpy restatement
(tests/util/flow_robust_model.py): the two stage entries, the whole estimator through fav_flow_rgb8, fav_flow_pairs_rgb8 and
fav_stream_next_frame_estimate, and fav_stylize -estimate_flow 1 -flow_eps.

Tolerance of the whole estimator: it is held to the fp64 model, and the bound is measured, not chosen: e32 = max|M32 - M64| of the
numpy model in fp32 against fp64 on the same input, computed here on the CPU at every run, and max|GPU - M64| <= 4 e32 (the nonlinearity
amplifies rounding, and the GPU's sqrt and division may differ from numpy's in the last place).  No floor, nothing measured against the
code under test.
Measured e32 (numpy on the CPU; options alpha 5, eps 0.3, 3 warps, 30 sweeps), in pixels: warped_pair(17, 23, 11) 4.4e-06,
(64, 64) 9.7e-06, (150, 203) 3.4e-05, two_motion_scene(96, 128, 1) 4.3e-05 -- so the bounds 4 e32 are 1.7e-05 .. 1.7e-04 px
(max|M64| 5.3 .. 13.2 px).  Measured on the MI355X: max|GPU - M64| = e32 on all four inputs, because the kernels came out BIT-EQUAL to
the fp32 model there (the flows, and the coefficients and weights of the stage entries too): the factor 4 is unused headroom.
The stage entries use the gate of tests/test_gpu_flow.py: max(4 e32, 2^-20 max(1, max|M64|))."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402
import flow_robust_model as R  # noqa: E402
from flow_testing import dev as _dev, gate_stage_robust as _stage_gate, run as _run, write_ppm as _write_ppm  # noqa: E402

from fav_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
VID = os.path.join(ROOT, "tests", "golden", "tiny_model.t7")
K = 6                    # the default sweeps_per_launch
SEED = 11
EPS = 0.3
INPUTS = [("warped", h, w) for h, w in M.SIZES] + [("scene", 96, 128)]


_cases = {}


def _case(kind, h, w):
    """(A, B, fp32 model flow, fp64 model flow) of an input, computed once and left unchanged"""
    if (kind, h, w) not in _cases:
        A, B = M.warped_pair(h, w, SEED) if kind == "warped" else R.two_motion_scene(h, w, 1)[:2]
        _cases[(kind, h, w)] = (A, B, R.flow(A, B, eps=EPS, dtype=np.float32), R.flow(A, B, eps=EPS, dtype=np.float64))
    return _cases[(kind, h, w)]


# ------------------------------------------------------------------------------------------------ 1. the stages
@pytest.mark.parametrize("h,w", M.SIZES)
def test_robust_coefficients_match_the_model(favlib, cuda, h, w):
    A, B = M.grey(synth.smooth_frame(h, w, 5)), M.grey(synth.smooth_frame(h, w, 6))
    for f0, name in ((synth.backward_flow(h, w, 8), "smooth flow"), (synth.random_flow(h, w, 9), "rough flow")):
        coef, wt = favlib.flow_coefficients_robust(_dev(A, cuda), _dev(B, cuda), _dev(f0, cuda), 5.0, EPS)
        c32, n32 = R.coefficients(A, B, f0, 5.0, EPS)
        c64, n64 = R.coefficients(A.astype(np.float64), B.astype(np.float64), f0, 5.0, EPS, dtype=np.float64)
        _stage_gate(coef.cpu().numpy(), c32, c64, f"coefficients {h}x{w}, {name}")
        _stage_gate(wt.cpu().numpy(), n32, n64, f"weights {h}x{w}, {name}")
        # (a, b, c) are the plain entry's, bit for bit
        plain = favlib.flow_coefficients(_dev(A, cuda), _dev(B, cuda), _dev(f0, cuda), 5.0).cpu().numpy()
        assert np.array_equal(coef.cpu().numpy()[..., :3], plain[..., :3])


_sweep_inputs = {}


def _sweep_case():
    if not _sweep_inputs:
        h, w = 150, 203
        rng = np.random.default_rng(21)
        A, B = (rng.standard_normal((2, h, w)) * 40 + 128).astype(np.float32)
        _sweep_inputs["x"] = (synth.random_flow(h, w, 22),) + R.coefficients(A, B, synth.random_flow(h, w, 23), 5.0, EPS)
    return _sweep_inputs["x"]


@pytest.mark.parametrize("iters", [1, K, K + 1, 2 * K + 3])
def test_robust_sweeps_do_not_depend_on_the_temporal_blocking(favlib, cuda, iters):
    """random (u0, v0), coefficients and weights of a rough flow at 150x203 (3 x 4 tiles of 52 with ragged last tiles; 2 x 2 at 16 per
    launch): sweeps_per_launch 1, 4, 6 and 16 bit for bit over the whole image, and against the model, which knows no tiles (a sweep has
    no division and no sqrt: every operation rounds as numpy's)"""
    f0, coef, wt = _sweep_case()
    d0, dc, dw = _dev(f0, cuda), _dev(coef, cuda), _dev(wt, cuda)
    single = favlib.flow_sweeps_robust(d0, dc, dw, iters, sweeps_per_launch=1).cpu().numpy()
    assert np.array_equal(d0.cpu().numpy(), f0) and np.array_equal(dw.cpu().numpy(), wt)          # the inputs are not written
    for k in (0, 4, 16):
        assert np.array_equal(favlib.flow_sweeps_robust(d0, dc, dw, iters, sweeps_per_launch=k).cpu().numpy(), single), k
    assert np.array_equal(single, R.sweeps(f0, coef, wt, iters))
    # weights of exactly 1/4 are the plain mean
    quarter = np.full_like(wt, 0.25)
    assert np.array_equal(favlib.flow_sweeps_robust(d0, dc, _dev(quarter, cuda), iters).cpu().numpy(), favlib.flow_sweeps(d0, dc, iters).cpu().numpy())


# ------------------------------------------------------------------------------------------------ 2. the whole estimator
@pytest.mark.parametrize("kind,h,w", INPUTS)
def test_robust_flow_matches_the_model(favlib, cuda, kind, h, w):
    import torch
    A, B, m32, m64 = _case(kind, h, w)
    a, b = _dev(A, cuda), _dev(B, cuda)
    got_t = favlib.flow_rgb8(a, b, smooth_eps=EPS)
    got = got_t.cpu().numpy()
    assert got.shape == (h, w, 2) and np.isfinite(got).all()
    e32 = float(np.abs(m32.astype(np.float64) - m64).max())
    err = float(np.abs(got.astype(np.float64) - m64).max())
    print(f"robust flow {kind} {h}x{w}: e32 {e32:.3e}  max|GPU - M64| {err:.3e}  bound {4 * e32:.3e}  max|M64| {np.abs(m64).max():.2f}  "
          f"bit-equal to M32: {np.array_equal(got, m32)}")
    assert err <= 4 * e32, (err, e32)
    for spl in (1, 6, 16):
        assert torch.equal(favlib.flow_rgb8(a, b, smooth_eps=EPS, sweeps_per_launch=spl), got_t), spl
    assert torch.equal(favlib.flow_rgb8(a, b, smooth_eps=EPS, alpha=5.0), got_t)                  # alpha 0 means 5 with the option on
    assert not torch.equal(favlib.flow_rgb8(a, b), got_t)


@pytest.mark.parametrize("n", [1, 2, 6])
def test_robust_pairs_equal_single_calls(favlib, cuda, n):
    import torch
    h, w = (150, 203) if n == 2 else (64, 64)
    pairs = [tuple(_dev(f, cuda) for f in M.warped_pair(h, w, 40 + k)) for k in range(n)]
    prev, cur = [p for p, _ in pairs], [c for _, c in pairs]
    bw, fw = favlib.flow_pairs(prev, cur, dict(smooth_eps=EPS))
    for k in range(n):
        assert torch.equal(bw[k], favlib.flow_rgb8(cur[k], prev[k], smooth_eps=EPS)), k
        assert torch.equal(fw[k], favlib.flow_rgb8(prev[k], cur[k], smooth_eps=EPS)), k
    if n > 1:
        assert not torch.equal(bw[0], bw[1])


def test_eps_zero_through_the_field_is_the_present_estimator(favlib, cuda):
    import torch
    for h, w in M.SIZES:
        A, B = _case("warped", h, w)[:2]
        a, b = _dev(A, cuda), _dev(B, cuda)
        assert torch.equal(favlib.flow_rgb8(a, b, smooth_eps=0.0), favlib.flow_rgb8(a, b)), (h, w)
    bw0, fw0 = favlib.flow_pairs([a], [b], dict(smooth_eps=0.0))
    bw1, fw1 = favlib.flow_pairs([a], [b])
    assert torch.equal(bw0[0], bw1[0]) and torch.equal(fw0[0], fw1[0])


# ------------------------------------------------------------------------------------------------ 3. poisoned state
def test_robust_flow_after_nan_poison(favlib, cuda, poison):
    import torch
    h, w = 150, 203
    A, B, m32, m64 = _case("warped", h, w)
    before = favlib.flow_rgb8(_dev(A, cuda), _dev(B, cuda), smooth_eps=EPS).cpu().numpy()
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    poison()
    a, b = _dev(A, cuda), _dev(B, cuda)
    o = favlib._flow_opts(dict(smooth_eps=EPS))
    nb = favlib.flow_workspace_bytes(w, h, smooth_eps=EPS)
    ws = torch.full(((nb + 3) // 4,), float("nan"), dtype=torch.float32, device=cuda)      # the workspace itself, too
    out = torch.full((h, w, 2), float("nan"), dtype=torch.float32, device=cuda)
    favlib._check(favlib.lib().fav_flow_rgb8(favlib._p(a), favlib._p(b), w, h, C.byref(o), favlib._p(out), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
    after = out.cpu().numpy()
    assert np.isfinite(after).all() and np.array_equal(after, before)
    assert float(np.abs(after.astype(np.float64) - m64).max()) <= 4 * float(np.abs(m32.astype(np.float64) - m64).max())
    # ... and the batch of one, both directions, with a 0x7f-filled workspace
    nbp = favlib.flow_pairs_workspace_bytes(w, h, 1, smooth_eps=EPS)
    wsp = torch.full((nbp,), 0x7f, dtype=torch.uint8, device=cuda)
    outs = [torch.full((h, w, 2), float("nan"), dtype=torch.float32, device=cuda) for _ in range(2)]
    one = lambda t: (C.c_void_p * 1)(t.data_ptr())
    favlib._check(favlib.lib().fav_flow_pairs_rgb8(one(b), one(a), 1, w, h, C.byref(o), one(outs[0]), one(outs[1]), favlib._p(wsp), C.c_size_t(nbp), favlib._stream()))
    assert np.array_equal(outs[0].cpu().numpy(), before) and torch.isfinite(outs[1]).all()


# ------------------------------------------------------------------------------------------------ 4. recovery on the device
def test_robust_flow_lowers_the_error_on_two_motions(favlib, cuda):
    """two_motion_scene(96, 128, 1): fp64 models 0.997 px (quadratic) and 0.628 px (robust); the device must show the same gain"""
    A, B, truth, valid = R.two_motion_scene(96, 128, 1)
    a, b = _dev(A, cuda), _dev(B, cuda)
    quad = R.scene_epe(favlib.flow_rgb8(a, b).cpu().numpy(), truth, valid)
    robust = R.scene_epe(favlib.flow_rgb8(a, b, smooth_eps=EPS).cpu().numpy(), truth, valid)
    print(f"GPU, mean endpoint error over the non-occluded interior: quadratic {quad:.4f} px, robust {robust:.4f} px, ratio {robust / quad:.3f}")
    assert robust <= 0.8 * quad


# ------------------------------------------------------------------------------------------------ 5. the executable
def test_cli_flow_eps_equals_the_stream_in_process(favlib, cuda, tmp_path):
    """fav_stylize -estimate_flow 1 -flow_eps 0.3 on three 64x64 frames of the two-motion scene's kind (a rectangle moving over a moving
    background): other files than with -flow_eps 0, and the files of Stream.next_frame_estimate(..., smooth_eps=0.3), byte for byte"""
    h, w, n = 64, 64, 3
    A, B = R.two_motion_scene(h, w, 1)[:2]
    frames = [A, B, A]                                                   # there and back
    for i, f in enumerate(frames):
        _write_ppm(str(tmp_path / f"frame_{i + 1:05d}.ppm"), f)
    common = [os.path.join(BIN, "fav_stylize"), "-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-model_vid", VID, "-model_img", "self",
              "-structure", "1", "-poll_settle", "0", "-poll_timeout", "20", "-estimate_flow", "1"]
    _run(common + ["-output_prefix", str(tmp_path / "eps" / "out"), "-flow_eps", "0.3"])
    _run(common + ["-output_prefix", str(tmp_path / "plain" / "out"), "-flow_eps", "0"])
    _run(common + ["-output_prefix", str(tmp_path / "none" / "out")])
    files = {k: [open(tmp_path / k / f"out-{i:05d}.png", "rb").read() for i in range(1, n + 1)] for k in ("eps", "plain", "none")}
    assert files["plain"] == files["none"]                               # the default is 0
    assert files["eps"][0] == files["plain"][0] and len(files["eps"][0]) > 100          # the first frame has no flow
    assert files["eps"][1] != files["plain"][1] and files["eps"][2] != files["plain"][2]
    net = favlib.Net(VID, 0)
    for key, opts in (("eps", dict(smooth_eps=0.3)), ("plain", {})):
        st = favlib.Stream(net, h, w)
        dev = [_dev(f, cuda) for f in frames]
        st.first_frame(dev[0])
        pngs = [favlib.png_encode(None, from_stream=st)]
        for i in (1, 2):
            st.next_frame_estimate(dev[i], dev[i - 1], use_structure=True, batched=True, **opts)
            pngs.append(favlib.png_encode(None, from_stream=st))
        st.close()
        assert pngs == files[key], key
