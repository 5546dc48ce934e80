"""The estimator's gradient-constancy data term (fav_flow_opts_ex.data_term = FAV_FLOW_DATA_GRADIENT) on the GPU against its numpy
restatement (tests/util/flow_grad_model.py): the two stage entries, the whole estimator through fav_flow_rgb8_ex, fav_flow_pairs_rgb8_ex
and fav_stylize -estimate_flow 1 -flow_grad 1, and the _ex entries with the option off against the entries of before.

Tolerances: the sweeps have no division and no square root and are held to the fp32 model bit for bit.  Everything else is held to the
fp64 model with a bound that is measured, not chosen: e32 = max|M32 - M64| of the numpy model in fp32 against fp64 on the same input,
computed here on the CPU at every run, and max|GPU - M64| <= 4 e32.  No floor, nothing measured against the code under test."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402
import flow_robust_model as R  # noqa: E402
import flow_grad_model as G  # noqa: E402
from flow_testing import dev as _dev, gate_4e32 as _gate, run as _run, write_ppm as _write_ppm  # noqa: E402

from fav_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
VID = os.path.join(ROOT, "tests", "golden", "tiny_model.t7")
SEED = 11
EPS = 0.3
INPUTS = [("warped", h, w, 0.0) for h, w in M.SIZES] + [("scene", 96, 128, 0.0), ("scene", 96, 128, EPS)]


_cases = {}


def _case(kind, h, w, eps):
    """(A, B, fp32 model flow, fp64 model flow) of an input, computed once and left unchanged"""
    if (kind, h, w, eps) not in _cases:
        A, B = M.warped_pair(h, w, SEED) if kind == "warped" else R.two_motion_scene(h, w, 1)[:2]
        _cases[(kind, h, w, eps)] = (A, B, G.flow(A, B, eps=eps, dtype=np.float32), G.flow(A, B, eps=eps, dtype=np.float64))
    return _cases[(kind, h, w, eps)]


def _planes(coef_t):
    """the binding's [5][H][W] -> the model's [H][W][5]"""
    return np.ascontiguousarray(coef_t.cpu().numpy().transpose(1, 2, 0))


# ------------------------------------------------------------------------------------------------ 1. the stages
@pytest.mark.parametrize("eps", [0.0, EPS])
@pytest.mark.parametrize("h,w", [(17, 23), (64, 64)])
def test_grad_stage_entries_match_the_model(favlib, cuda, h, w, eps):
    """17x23: a partial tile, every pixel within two of a border (both nested clamps); 64x64: exactly one region"""
    A, B = M.grey(synth.smooth_frame(h, w, 5)), M.grey(synth.smooth_frame(h, w, 6))
    for f0, name in ((synth.backward_flow(h, w, 8), "smooth flow"), (synth.random_flow(h, w, 9), "rough flow")):
        d0 = _dev(f0, cuda)
        got = favlib.flow_coefficients_grad(_dev(A, cuda), _dev(B, cuda), d0, 8.0, eps)
        m32 = G.coefficients(A, B, f0, 8.0, eps)
        m64 = G.coefficients(A.astype(np.float64), B.astype(np.float64), f0, 8.0, eps, dtype=np.float64)
        if eps:
            (coef_t, wt_t), (c32, n32), (c64, n64) = got, m32, m64
            _gate(wt_t.cpu().numpy(), n32, n64, f"weights {h}x{w}, {name}")
            assert np.array_equal(wt_t.cpu().numpy(), favlib.flow_coefficients_robust(_dev(A, cuda), _dev(B, cuda), d0, 8.0, eps)[1].cpu().numpy())
        else:
            coef_t, c32, c64, wt_t, n32 = got, m32, m64, None, None
        assert tuple(coef_t.shape) == (5, h, w)
        _gate(_planes(coef_t), c32, c64, f"coefficients {h}x{w}, eps {eps}, {name}")
        # the sweeps: from the MODEL's fp32 coefficients, so that the comparison is bit for bit whatever the divisions did
        dc = _dev(np.ascontiguousarray(c32.transpose(2, 0, 1)), cuda)
        dw = _dev(n32, cuda) if eps else None
        start = synth.random_flow(h, w, 22)
        ds = _dev(start, cuda)
        for iters in (1, 7, 15):
            single = favlib.flow_sweeps_grad(ds, dc, iters, sweeps_per_launch=1, weights=dw).cpu().numpy()
            assert np.array_equal(single, G.sweeps(start, c32, iters, weights=n32)), (iters, name)
            for k in (0, 4, 16):
                assert np.array_equal(favlib.flow_sweeps_grad(ds, dc, iters, sweeps_per_launch=k, weights=dw).cpu().numpy(), single), (iters, k)
        assert np.array_equal(ds.cpu().numpy(), start)          # the input is not written


# ------------------------------------------------------------------------------------------------ 2., 3. the whole estimator
@pytest.mark.parametrize("kind,h,w,eps", INPUTS)
def test_grad_flow_matches_the_model(favlib, cuda, kind, h, w, eps):
    import torch
    A, B, m32, m64 = _case(kind, h, w, eps)
    a, b = _dev(A, cuda), _dev(B, cuda)
    got_t = favlib.flow_rgb8(a, b, data_term=1, smooth_eps=eps)
    got = got_t.cpu().numpy()
    assert got.shape == (h, w, 2)
    _gate(got, m32, m64, f"gradient-term flow {kind} {h}x{w} eps {eps}")
    for spl in (1, 6, 16):
        assert torch.equal(favlib.flow_rgb8(a, b, gradient_data=True, smooth_eps=eps, sweeps_per_launch=spl), got_t), spl
    assert torch.equal(favlib.flow_rgb8(a, b, data_term=1, smooth_eps=eps, alpha=8.0), got_t)          # alpha 0 means 8 with the option on
    assert not torch.equal(favlib.flow_rgb8(a, b, smooth_eps=eps), got_t)


# ------------------------------------------------------------------------------------------------ 4. poisoned state
def test_grad_flow_after_nan_poison(favlib, cuda, poison):
    import torch
    h, w = 150, 203
    A, B, m32, m64 = _case("warped", h, w, 0.0)
    before = favlib.flow_rgb8(_dev(A, cuda), _dev(B, cuda), data_term=1).cpu().numpy()
    before_eps = favlib.flow_rgb8(_dev(A, cuda), _dev(B, cuda), data_term=1, smooth_eps=EPS).cpu().numpy()
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    poison()
    a, b = _dev(A, cuda), _dev(B, cuda)
    for opts, want in ((dict(data_term=1), before), (dict(data_term=1, smooth_eps=EPS), before_eps)):
        o = favlib._flow_opts_ex(opts)
        nb = favlib.flow_workspace_bytes(w, h, **opts)
        ws = torch.full(((nb + 3) // 4,), float("nan"), dtype=torch.float32, device=cuda)      # the workspace itself, too
        out = torch.full((h, w, 2), float("nan"), dtype=torch.float32, device=cuda)
        favlib._check(favlib.lib().fav_flow_rgb8_ex(favlib._p(a), favlib._p(b), w, h, C.byref(o), favlib._p(out), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
        after = out.cpu().numpy()
        assert np.isfinite(after).all() and np.array_equal(after, want), opts
    assert float(np.abs(before.astype(np.float64) - m64).max()) <= 4 * float(np.abs(m32.astype(np.float64) - m64).max())


# ------------------------------------------------------------------------------------------------ 5. the batch
def test_grad_pairs_equal_single_calls(favlib, cuda):
    import torch
    h, w = 150, 203
    pairs = [tuple(_dev(f, cuda) for f in M.warped_pair(h, w, 40 + k)) for k in range(2)]
    prev, cur = [p for p, _ in pairs], [c for _, c in pairs]
    for opts in (dict(data_term=1), dict(data_term=1, smooth_eps=EPS)):
        bw, fw = favlib.flow_pairs(prev, cur, opts)
        for k in range(2):
            assert torch.equal(bw[k], favlib.flow_rgb8(cur[k], prev[k], **opts)), (k, opts)
            assert torch.equal(fw[k], favlib.flow_rgb8(prev[k], cur[k], **opts)), (k, opts)
        assert not torch.equal(bw[0], bw[1])
    # one image in two slots: (p0, c0) and (c0, p0) -- slot 1 is slot 0 with the directions exchanged
    bw, fw = favlib.flow_pairs([prev[0], cur[0]], [cur[0], prev[0]], dict(data_term=1))
    assert torch.equal(bw[0], fw[1]) and torch.equal(fw[0], bw[1])
    assert torch.equal(fw[0], favlib.flow_rgb8(prev[0], cur[0], data_term=1))


# ------------------------------------------------------------------------------------------------ 6. recovery on the device
def test_grad_flow_recovers_a_relit_shift(favlib, cuda):
    """flow_model.shifted_pair(1, 96, 128), B relit 0.8 B + 10: fp64 models 6.69 px (brightness) and 0.280 px (gradients).  The option
    must bring the device's estimate to <= 0.6 px, and without it the same pair must stay >= 3 px: the feature, not the input, passes."""
    A, B, t = M.shifted_pair(1, 96, 128)
    a, b = _dev(A, cuda), _dev(G.relight(B, 0.8, 10.0), cuda)
    bright = M.interior_epe(favlib.flow_rgb8(a, b).cpu().numpy(), t)
    grad = M.interior_epe(favlib.flow_rgb8(a, b, data_term=1).cpu().numpy(), t)
    print(f"GPU, mean interior endpoint error of the relit pair: brightness {bright:.4f} px, gradients {grad:.4f} px")
    assert grad <= 0.6 and bright >= 3.0


# ------------------------------------------------------------------------------------------------ 7. the option off
def test_ex_entries_with_data_term_0_are_the_old_entries(favlib, cuda):
    import torch
    L = favlib.lib()
    one = lambda t: (C.c_void_p * 1)(t.data_ptr())
    for h, w in M.SIZES:
        A, B = _case("warped", h, w, 0.0)[:2]
        a, b = _dev(A, cuda), _dev(B, cuda)
        for opts in ({}, dict(smooth_eps=EPS)):
            old_o, ex_o = favlib._flow_opts(opts), favlib._flow_opts_ex(dict(opts, data_term=0))
            nb = L.fav_flow_workspace_bytes(w, h, C.cast(C.pointer(old_o), C.c_void_p))
            assert nb == favlib.flow_workspace_bytes(w, h, data_term=0, **opts)
            ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
            old, ex = torch.empty((h, w, 2), dtype=torch.float32, device=cuda), torch.empty((h, w, 2), dtype=torch.float32, device=cuda)
            favlib._check(L.fav_flow_rgb8(favlib._p(a), favlib._p(b), w, h, C.byref(old_o), favlib._p(old), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
            favlib._check(L.fav_flow_rgb8_ex(favlib._p(a), favlib._p(b), w, h, C.byref(ex_o), favlib._p(ex), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
            assert torch.equal(old, ex) and torch.isfinite(old).all(), (h, w, opts)
            # the batch of one, both directions
            nbp = L.fav_flow_pairs_workspace_bytes(w, h, 1, C.cast(C.pointer(old_o), C.c_void_p))
            assert nbp == favlib.flow_pairs_workspace_bytes(w, h, 1, data_term=0, **opts)
            wsp = torch.empty(nbp, dtype=torch.uint8, device=cuda)
            o4 = [torch.empty((h, w, 2), dtype=torch.float32, device=cuda) for _ in range(4)]
            favlib._check(L.fav_flow_pairs_rgb8(one(a), one(b), 1, w, h, C.byref(old_o), one(o4[0]), one(o4[1]), favlib._p(wsp), C.c_size_t(nbp), favlib._stream()))
            favlib._check(L.fav_flow_pairs_rgb8_ex(one(a), one(b), 1, w, h, C.byref(ex_o), one(o4[2]), one(o4[3]), favlib._p(wsp), C.c_size_t(nbp), favlib._stream()))
            assert torch.equal(o4[0], o4[2]) and torch.equal(o4[1], o4[3]) and torch.equal(o4[1], old), (h, w, opts)


# ------------------------------------------------------------------------------------------------ 8. the executable
def test_cli_flow_grad_keeps_the_mask_on_a_relit_clip(favlib, cuda, tmp_path):
    """fav_stylize -estimate_flow 1 -flow_grad 1 on three 64x64 frames: shifted_pair(1, 64, 64)'s A, its B relit 0.8 B + 10, and A relit
    B + 25.  Three PNGs, the files of Stream.next_frame_estimate(..., data_term=1), and other files than without the flag.
    The share of reliable pixels in frame 2's mask (both flows from flow_pairs, then the consistency check with the frame, as -structure 1
    does): with the two fp64 models and the oracle's checker on the CPU it is 0.167 with the brightness term and 0.505 with the gradient
    term; required on the device: at least twice the share without the flag."""
    h, w, n = 64, 64, 3
    A, B, _ = M.shifted_pair(1, h, w)
    frames = [A, G.relight(B, 0.8, 10.0), G.relight(A, 1.0, 25.0)]
    for i, f in enumerate(frames):
        _write_ppm(str(tmp_path / f"frame_{i + 1:05d}.ppm"), f)
    common = [os.path.join(BIN, "fav_stylize"), "-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-model_vid", VID, "-model_img", "self",
              "-structure", "1", "-poll_settle", "0", "-poll_timeout", "20", "-estimate_flow", "1"]
    _run(common + ["-output_prefix", str(tmp_path / "grad" / "out"), "-flow_grad", "1"])
    _run(common + ["-output_prefix", str(tmp_path / "plain" / "out"), "-flow_grad", "0"])
    files = {k: [open(tmp_path / k / f"out-{i:05d}.png", "rb").read() for i in range(1, n + 1)] for k in ("grad", "plain")}
    assert all(len(f) > 100 for f in files["grad"])
    assert files["grad"][0] == files["plain"][0]                         # the first frame has no flow
    assert files["grad"][1] != files["plain"][1] and files["grad"][2] != files["plain"][2]
    net = favlib.Net(VID, 0)
    dev = [_dev(f, cuda) for f in frames]
    for key, opts in (("grad", dict(data_term=1)), ("plain", {})):
        st = favlib.Stream(net, h, w)
        st.first_frame(dev[0])
        pngs = [favlib.png_encode(None, from_stream=st)]
        for i in (1, 2):
            st.next_frame_estimate(dev[i], dev[i - 1], use_structure=True, batched=True, **opts)
            pngs.append(favlib.png_encode(None, from_stream=st))
        st.close()
        assert pngs == files[key], key
    share = {}
    for key, opts in (("grad", dict(data_term=1)), ("plain", {})):
        bw, fw = favlib.flow_pairs([dev[0]], [dev[1]], opts)
        share[key] = float((favlib.consistency(bw[0], fw[0], dev[1]) == 255).float().mean())
    print(f"reliable share of frame 2: brightness {share['plain']:.3f}, gradients {share['grad']:.3f}")
    assert share["grad"] >= 2 * share["plain"] and share["grad"] > 0
