"""The estimator's block-matching prior (fav_flow_opts_ex2.match_beta) on the GPU against its numpy restatement
(tests/util/flow_match_model.py): the three stage entries, the whole estimator through fav_flow_rgb8_ex2, fav_flow_pairs_rgb8_ex2 and
fav_stylize -estimate_flow 1 -flow_match 1, and the _ex2 entries with the option off against the _ex entries.

Tolerances: the match fields and the confidence are integers and must EQUAL the model's.  Everything with a division is held to the fp64
model with a bound that is measured, not chosen: e32 = max|M32 - M64| of the numpy model in fp32 against fp64 on the same input, computed
here on the CPU at every run, and max|GPU - M64| <= 4 e32.  The prior's gate is a threshold: the inputs are chosen so that the fp32 and
the fp64 MODEL agree on it at every pixel of every warp, which each test asserts on the CPU before it looks at the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402
import flow_match_model as P  # noqa: E402
from flow_testing import dev as _dev, gate_4e32 as _gate, run as _run, write_ppm as _write_ppm  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
VID = os.path.join(ROOT, "tests", "golden", "tiny_model.t7")
EPS = 0.3
SMALL_SCENE = (64, 64, 2, (22, 42, 20, 40), (9.0, -6.0), (1.0, 0.0))          # a 20 x 20 object moving (9, -6) over a background moving (1, 0)


def _scene(name):
    return P.scene(*SMALL_SCENE) if name == "64x64" else P.half_scene()


_cases = {}


def _case(name, eps, grad):
    """(A, B, fp32 model flow, fp64 model flow) of a scene with the prior (64x64: R 16; 96x128: R 8), computed once and left unchanged;
    asserts that the two models agree on the gate at every pixel of every warp and that the gate is on somewhere"""
    key = (name, eps, grad)
    if key not in _cases:
        A, B = _scene(name)[:2]
        radius = 16 if name == "64x64" else 8
        t32, t64 = [], []
        m32 = P.flow(A, B, eps=eps, grad=grad, radius=radius, dtype=np.float32, trace=t32)
        m64 = P.flow(A, B, eps=eps, grad=grad, radius=radius, dtype=np.float64, trace=t64)
        assert len(t32) == len(t64) > 0
        on_somewhere = False
        for i, ((d32, tau), (d64, _)) in enumerate(zip(t32, t64)):
            assert np.array_equal(d32 > np.float32(tau), d64 > tau), f"{key}: the fp32 and fp64 models disagree on the gate in warp {i}"
            on_somewhere |= bool((d64 > tau).any())
        assert on_somewhere, key
        _cases[key] = (A, B, m32, m64)
    return _cases[key]


def _planes(t):
    """the binding's [C][H][W] -> the model's [H][W][C]"""
    return np.ascontiguousarray(t.cpu().numpy().transpose(1, 2, 0))


def _prior_planes(d, m):
    """the model's (d [H][W][2], m [H][W]) -> the entry's [3][H][W] fp32"""
    return np.ascontiguousarray(np.concatenate([np.asarray(d, np.float32).transpose(2, 0, 1), np.asarray(m, np.float32)[None]], 0))


# ------------------------------------------------------------------------------------------------ 1. matching and the check
def _match_inputs():
    A, B = M.warped_pair(17, 23, 11, std=3.0)
    yield "warped 17x23 (smaller than the search window: every clamp is live)", M.grey(A), M.grey(B), 16
    A, B = M.warped_pair(64, 64, 12, std=4.0)
    yield "warped 64x64, R 16 (one tile, rows beyond the image)", M.grey(A), M.grey(B), 16
    A, B = M.warped_pair(75, 101, 13, std=3.0)
    yield "warped 75x101, R 5 (four column tiles, two row tiles, partial ones)", M.grey(A), M.grey(B), 5
    seed, rect, fg, bg = P.LARGE[0]
    A, B = P.scene(P.SCENE_H, P.SCENE_W, seed, rect, fg, bg)[:2]
    yield "scene 1 cropped to 96x128, R 16", M.grey(A[48:144, 64:192]), M.grey(B[48:144, 64:192]), 16
    yield "scene 1 cropped to 96x128, R 32 (the largest window)", M.grey(A[48:144, 64:192]), M.grey(B[48:144, 64:192]), 32


@pytest.mark.parametrize("case", range(5))
def test_match_and_check_equal_the_model(favlib, cuda, case):
    import torch
    name, gA, gB, radius = list(_match_inputs())[case]
    h, w = gA.shape
    want_ab, want_ba = P.match(gA, gB, radius), P.match(gB, gA, radius)
    d_ab, d_ba = favlib.flow_match(_dev(gA, cuda), _dev(gB, cuda), radius)
    assert d_ab.dtype == torch.int16 and tuple(d_ab.shape) == (h, w, 2)
    got_ab, got_ba = d_ab.cpu().numpy().astype(np.int64), d_ba.cpu().numpy().astype(np.int64)
    print(f"{name}: {int((got_ab != want_ab).any(-1).sum())} + {int((got_ba != want_ba).any(-1).sum())} of {h * w} pixels differ; "
          f"|d| up to {np.abs(want_ab).max()}, {len(np.unique(want_ab.reshape(-1, 2), axis=0))} distinct displacements")
    assert np.array_equal(got_ab, want_ab) and np.array_equal(got_ba, want_ba), name
    for a, b, wa, wb in ((d_ab, d_ba, want_ab, want_ba), (d_ba, d_ab, want_ba, want_ab)):
        want_m = P.check(wa, wb)
        assert np.array_equal(favlib.flow_match_check(a, b).cpu().numpy(), want_m.astype(np.float32)), name
        assert np.array_equal(favlib.flow_match_check(a, b, want_prior=True).cpu().numpy(), _prior_planes(wa, want_m)), name
        assert 0 < want_m.mean() < 1 or h < 20, name          # (both outcomes occur)


# ------------------------------------------------------------------------------------------------ 2. the coefficients with a prior
@pytest.mark.parametrize("level0", [False, True])
@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("eps", [0.0, EPS])
def test_prior_coefficients_match_the_model(favlib, cuda, eps, grad, level0):
    """the 64x64 scene's grey planes with the match field of its own size (tau 1) or, level0, with level 1's field read through the parent
    sample (tau 2)"""
    A, B = _scene("64x64")[:2]
    pa, pb = M.pyramid(A, 2), M.pyramid(B, 2)
    gA, gB = pa[0], pb[0]
    src = 1 if level0 else 0
    d_ab, d_ba = P.match(pa[src], pb[src], 16), P.match(pb[src], pa[src], 16)
    m = P.check(d_ab, d_ba)
    # around a flow that is the prior's own displacement plus noise of 1.5 px: the gate is on at some pixels and off at others
    d_here = P.prior_level0(d_ab, m, 64, 64, np.float64)[0] if level0 else d_ab
    f0 = (d_here + 1.5 * np.random.default_rng(8).standard_normal((64, 64, 2))).astype(np.float32)
    tau, alpha = (P.TAU0 if level0 else P.TAU), P.default_alpha(eps, grad)
    res = {}
    for dt in (np.float32, np.float64):
        d, mm = P.prior_level0(d_ab, m, 64, 64, dt) if level0 else (d_ab.astype(dt), m.astype(dt))
        on, dist = P.gate(d, f0, tau, dt)
        r = P.coefficients(gA.astype(dt), gB.astype(dt), f0, d, mm, alpha, P.BETA, tau, eps, grad, dt)
        res[dt] = (r if eps else (r, None)) + (on, on & (mm > 0))
    assert np.array_equal(res[np.float32][2], res[np.float64][2]) and not res[np.float64][2].all()          # the two models agree on the gate, which is off somewhere
    assert res[np.float64][3].any()                                                                          # ... and the prior acts somewhere
    got = favlib.flow_coefficients_prior(_dev(gA, cuda), _dev(gB, cuda), _dev(f0, cuda), _dev(_prior_planes(d_ab, m), cuda), alpha, P.BETA, tau, eps, int(grad))
    coef_t, wt_t = got if eps else (got, None)
    assert tuple(coef_t.shape) == (5, 64, 64)
    _gate(_planes(coef_t), res[np.float32][0], res[np.float64][0], f"prior coefficients eps {eps} grad {grad} level0 {level0}")
    if eps:
        _gate(wt_t.cpu().numpy(), res[np.float32][1], res[np.float64][1], "weights")
    # without the prior's pull the coefficients are others
    far = favlib.flow_coefficients_prior(_dev(gA, cuda), _dev(gB, cuda), _dev(f0, cuda), _dev(_prior_planes(d_ab, m), cuda), alpha, P.BETA, 1e9, eps, int(grad))
    assert not np.array_equal(_planes(far[0] if eps else far), _planes(coef_t))


# ------------------------------------------------------------------------------------------------ 3. the whole estimator
@pytest.mark.parametrize("name,eps,grad", [("64x64", 0.0, False), ("64x64", EPS, False), ("64x64", 0.0, True), ("64x64", EPS, True), ("96x128", 0.0, False)])
def test_prior_flow_matches_the_model(favlib, cuda, name, eps, grad):
    import torch
    A, B, m32, m64 = _case(name, eps, grad)
    a, b = _dev(A, cuda), _dev(B, cuda)
    opts = dict(match_beta=-1, match_radius=16 if name == "64x64" else 8, smooth_eps=eps, data_term=int(grad))
    got_t = favlib.flow_rgb8(a, b, **opts)
    got = got_t.cpu().numpy()
    assert got.shape == A.shape[:2] + (2,)
    _gate(got, m32, m64, f"flow with the prior, {name} eps {eps} grad {grad}")
    for spl in (1, 6, 16):
        assert torch.equal(favlib.flow_rgb8(a, b, **dict(opts, sweeps_per_launch=spl)), got_t), spl
    assert torch.equal(favlib.flow_rgb8(a, b, **dict(opts, match_beta=P.BETA)), got_t)          # a negative beta means 225
    if name == "64x64":
        assert torch.equal(favlib.flow_rgb8(a, b, **dict(opts, match_radius=0)), got_t)         # radius 0 means 16
    assert not torch.equal(favlib.flow_rgb8(a, b, smooth_eps=eps, data_term=int(grad)), got_t)


def test_prior_recovers_the_object_on_the_device(favlib, cuda):
    """flow_match_model.half_scene() (96 x 128, a 20 x 20 object moving (11, -7) over a background moving (1, 0); 3 levels), R 8.  fp64
    models, mean endpoint error on the object: 16.06 px plain, 4.35 px with the prior.  Required on the device: the model's figure (to
    1e-3 px: the flow itself is held to 4 e32 above) and at most half the plain estimator's, which must itself stay above 8 px -- the
    feature, not the input, passes."""
    A, B, truth, valid, obj = P.half_scene()
    a, b = _dev(A, cuda), _dev(B, cuda)
    plain = P.scene_errors(favlib.flow_rgb8(a, b).cpu().numpy(), truth, valid, obj)
    prior = P.scene_errors(favlib.flow_rgb8(a, b, match_beta=-1, match_radius=8).cpu().numpy(), truth, valid, obj)
    model = P.scene_errors(_case("96x128", 0.0, False)[3], truth, valid, obj)
    print(f"GPU, object / background error: plain {plain[0]:.4f} / {plain[1]:.4f} px, prior {prior[0]:.4f} / {prior[1]:.4f} px; fp64 model {model[0]:.4f} / {model[1]:.4f} px")
    assert abs(prior[0] - model[0]) <= 1e-3 and abs(prior[1] - model[1]) <= 1e-3
    assert plain[0] >= 8.0 and prior[0] <= 0.5 * plain[0]


# ------------------------------------------------------------------------------------------------ 4. poisoned state
def test_prior_flow_after_nan_poison(favlib, cuda, poison):
    import torch
    A, B, m32, m64 = _case("64x64", 0.0, False)
    h, w = A.shape[:2]
    all_opts = (dict(match_beta=-1), dict(match_beta=-1, smooth_eps=EPS, data_term=1))
    before = [favlib.flow_rgb8(_dev(A, cuda), _dev(B, cuda), **o).cpu().numpy() for o in all_opts]
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    poison()
    a, b = _dev(A, cuda), _dev(B, cuda)
    for opts, want in zip(all_opts, before):
        o = favlib._flow_opts_ex2(opts)
        nb = favlib.flow_workspace_bytes(w, h, **opts)
        ws = torch.full(((nb + 3) // 4,), float("nan"), dtype=torch.float32, device=cuda)      # the workspace itself, too
        out = torch.full((h, w, 2), float("nan"), dtype=torch.float32, device=cuda)
        favlib._check(favlib.lib().fav_flow_rgb8_ex2(favlib._p(a), favlib._p(b), w, h, C.byref(o), favlib._p(out), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
        after = out.cpu().numpy()
        assert np.isfinite(after).all() and np.array_equal(after, want), opts
    assert float(np.abs(before[0].astype(np.float64) - m64).max()) <= 4 * float(np.abs(m32.astype(np.float64) - m64).max())


# ------------------------------------------------------------------------------------------------ 5. the batch
@pytest.mark.parametrize("n", [1, 2, 6])
def test_prior_pairs_equal_single_calls(favlib, cuda, n):
    import torch
    h, w, _, rect, fg, bg = SMALL_SCENE
    pairs = [tuple(_dev(f, cuda) for f in P.scene(h, w, 20 + k, rect, (fg[0] - k, fg[1] + k), bg)[:2]) for k in range(n)]
    prev, cur = [p for p, _ in pairs], [c for _, c in pairs]
    for opts in (dict(match_beta=-1), dict(match_beta=-1, data_term=1, smooth_eps=EPS)) if n == 2 else (dict(match_beta=-1),):
        bw, fw = favlib.flow_pairs(prev, cur, opts)
        for k in range(n):
            assert torch.equal(bw[k], favlib.flow_rgb8(cur[k], prev[k], **opts)), (k, opts)
            assert torch.equal(fw[k], favlib.flow_rgb8(prev[k], cur[k], **opts)), (k, opts)
        assert not torch.equal(bw[0], favlib.flow_pairs(prev, cur, {k: v for k, v in opts.items() if k != "match_beta"})[0][0])
    if n == 2:      # one image in two slots: slot 1 is slot 0 with the directions exchanged
        bw, fw = favlib.flow_pairs([prev[0], cur[0]], [cur[0], prev[0]], dict(match_beta=-1))
        assert torch.equal(bw[0], fw[1]) and torch.equal(fw[0], bw[1])


# ------------------------------------------------------------------------------------------------ 6. the option off
def test_ex2_entries_with_match_beta_0_are_the_ex_entries(favlib, cuda):
    import torch
    L = favlib.lib()
    one = lambda t: (C.c_void_p * 1)(t.data_ptr())
    void = lambda o: C.cast(C.pointer(o), C.c_void_p)
    for h, w in M.SIZES:
        A, B = M.warped_pair(h, w, 11)
        a, b = _dev(A, cuda), _dev(B, cuda)
        for opts in ({}, dict(smooth_eps=EPS), dict(data_term=1), dict(data_term=1, smooth_eps=EPS)):
            ex_o, ex2_o = favlib._flow_opts_ex(opts), favlib._flow_opts_ex2(dict(opts, match_beta=0.0, match_radius=9))
            nb = L.fav_flow_workspace_bytes_ex(w, h, void(ex_o))
            assert nb == L.fav_flow_workspace_bytes_ex2(w, h, void(ex2_o))
            ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
            ex, ex2 = torch.empty((h, w, 2), dtype=torch.float32, device=cuda), torch.empty((h, w, 2), dtype=torch.float32, device=cuda)
            favlib._check(L.fav_flow_rgb8_ex(favlib._p(a), favlib._p(b), w, h, C.byref(ex_o), favlib._p(ex), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
            favlib._check(L.fav_flow_rgb8_ex2(favlib._p(a), favlib._p(b), w, h, C.byref(ex2_o), favlib._p(ex2), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
            assert torch.equal(ex, ex2) and torch.isfinite(ex).all(), (h, w, opts)
            nbp = L.fav_flow_pairs_workspace_bytes_ex(w, h, 1, void(ex_o))
            assert nbp == L.fav_flow_pairs_workspace_bytes_ex2(w, h, 1, void(ex2_o))
            wsp = torch.empty(nbp, dtype=torch.uint8, device=cuda)
            o4 = [torch.empty((h, w, 2), dtype=torch.float32, device=cuda) for _ in range(4)]
            favlib._check(L.fav_flow_pairs_rgb8_ex(one(a), one(b), 1, w, h, C.byref(ex_o), one(o4[0]), one(o4[1]), favlib._p(wsp), C.c_size_t(nbp), favlib._stream()))
            favlib._check(L.fav_flow_pairs_rgb8_ex2(one(a), one(b), 1, w, h, C.byref(ex2_o), one(o4[2]), one(o4[3]), favlib._p(wsp), C.c_size_t(nbp), favlib._stream()))
            assert torch.equal(o4[0], o4[2]) and torch.equal(o4[1], o4[3]) and torch.equal(o4[1], ex), (h, w, opts)


# ------------------------------------------------------------------------------------------------ 7. the executable
def test_cli_flow_match_is_the_streams_estimate(favlib, cuda, tmp_path):
    """fav_stylize -estimate_flow 1 -flow_match 1 on three 64x64 frames (the 64x64 scene's A, B, A): three PNGs, the files of
    Stream.next_frame_estimate(..., match_beta=-1), and other files than without the flag"""
    h, w, n = 64, 64, 3
    A, B = _scene("64x64")[:2]
    frames = [A, B, A]
    for i, f in enumerate(frames):
        _write_ppm(str(tmp_path / f"frame_{i + 1:05d}.ppm"), f)
    common = [os.path.join(BIN, "fav_stylize"), "-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-model_vid", VID, "-model_img", "self",
              "-structure", "1", "-poll_settle", "0", "-poll_timeout", "20", "-estimate_flow", "1"]
    _run(common + ["-output_prefix", str(tmp_path / "match" / "out"), "-flow_match", "1"])
    _run(common + ["-output_prefix", str(tmp_path / "plain" / "out"), "-flow_match", "0"])
    files = {k: [open(tmp_path / k / f"out-{i:05d}.png", "rb").read() for i in range(1, n + 1)] for k in ("match", "plain")}
    assert all(len(f) > 100 for f in files["match"])
    assert files["match"][0] == files["plain"][0]                        # the first frame has no flow
    assert files["match"][1] != files["plain"][1] and files["match"][2] != files["plain"][2]
    net = favlib.Net(VID, 0)
    dev = [_dev(f, cuda) for f in frames]
    for key, opts in (("match", dict(match_beta=-1)), ("plain", {})):
        st = favlib.Stream(net, h, w)
        st.first_frame(dev[0])
        pngs = [favlib.png_encode(None, from_stream=st)]
        for i in (1, 2):
            st.next_frame_estimate(dev[i], dev[i - 1], use_structure=True, batched=True, **opts)
            pngs.append(favlib.png_encode(None, from_stream=st))
        st.close()
        assert pngs == files[key], key
