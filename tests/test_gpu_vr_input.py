"""What a cube face's network reads (csrc/vr.cpp vr_face: the neighbour table, add_border = rotate_kernel + warp + accum_kernel,
flo_to_lua_kernel and the flow warp, vr_prior_kernel, prep_prior_kernel, the hipMemsetAsync branch of -create_inconsistent_border, the
"single" rule of -create_inconsistent), looked at directly: fav_vr_get_f32 kinds 5, 6, 7 and fav_vr_get_padded_input_f32
(include/fav_vr_state.h) against tests/util/vr_input_model.py, which is written from the reference's Lua.

Every case is ONE face on a handle the test has prepared (six blended faces of a previous frame and the raw faces before `mode` through
fav_vr_set_f32).  Per case, EQUAL (every stage is a copy, a selection or a fixed sequence of single fp32 roundings; kernels_vr.hip is
built with -ffp-contract=off; -0.0 == +0.0):
  certainty  get(5)   == vr_oracle's plane (as tests/test_gpu_vr_post.py::test_certainty_plane_260_equals_oracle holds it; under the
                         CPU border the oracle's _cert is given the static masks of that border, warps of ones by the library's
                         operator); the model takes the GPU's plane as its certainty
  border     get(6)   == model.border with the library's own warp operator (fav_warp_bdhw_f32, pinned to the reference's kernel by
                         tests/test_gpu_parity.py) on the model's rotated faces and fav_vr_map_host's maps
  prior      get(7)   == model.prior on the GPU's own border and certainty, lfw = the library's warp of the previous face
  input               == model.padded_input on the GPU's own prior and certainty, all (H + 32) (W + 32) 8 floats
and border and prior within 1e-5 max(1, max |face|) of the pure-CPU values (the project's bound for whatever contains the warp), and
the same bits again after the handle's buffers have been dirtied by another face and a fav_vr_finish_frame -- every case of this
file, single images and both -create_inconsistent options included.

Sizes: 64 (one block per row) and 260 (rotate_kernel's second block, ragged; padded rows of 292 > 256).

Sphere faces at 64: the assertion of tests/test_cpu_vr_input.py::test_sphere_border_per_mode on the GPU's border, with the bound
recorded in tests/util/vr_input_model.py (SPHERE_MEASURED: twice the model's own deviation)."""
import copy
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import vr_check_inputs as VI  # noqa: E402
import vr_input_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
OV = 24
TOL = 1e-5
MSG6 = r"libfav error -1: fav_vr_get_f32: kind 6 \(border sum\)"
MSG7 = r"libfav error -1: fav_vr_get_f32: kind 7 \(prior\)"
MSGP = r"libfav error -1: fav_vr_get_padded_input_f32: no face has been assembled yet"


def T(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev) if a is not None else None


@pytest.fixture(scope="module")
def net(favlib, golden_dir):
    n = favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)
    assert n.input_pad() == 16
    return n


@pytest.fixture(scope="module")
def V(oracle):
    import vr_oracle
    return vr_oracle


_STATIC = {}


def _static(favlib, V, cuda, n, border):
    """fav_vr_map_host's maps, the library's warp operator as the model's warp_fn, the model's masks and gradient masks -- once per size
    and border mode.  Under the reference's border the masks must be vr_oracle's, bit for bit."""
    key = (n, border)
    if key not in _STATIC:
        maps = {k: favlib.vr_map_host(q, n, n, OV) for q, k in enumerate((M.L, M.R, M.T, M.B))}
        warp = lambda img, mp: favlib.warp(T(np.asarray(img, F), cuda), T(mp, cuda), border).cpu().numpy()
        masks = M.static_masks(warp, maps)
        if border == favlib.BORDER_STN:
            ref = _oracle(V, n, 7, False, 1)
            for k, want in ((M.L, ref.mask_left), (M.R, ref.mask_right), (M.T, ref.mask_top), (M.B, ref.mask_bottom),
                            ("all", ref.mask_all), ("all_div", ref.mask_all_div)):
                assert np.array_equal(masks[k], want[0]), f"static mask {k} at {n}"
        _STATIC[key] = (maps, warp, masks, M.grad_masks(n, n, OV, OV))
    return _STATIC[key]


@functools.lru_cache(maxsize=None)
def _oracle(V, n, r, inconsistent, inconsistent_border):
    return V.VRStylizer(None, n, n, overlap_w=OV, overlap_h=OV, min_filter_r=r, create_inconsistent=bool(inconsistent),
                        create_inconsistent_border=bool(inconsistent_border))


_CPU_MASKS = {}


def _cpu_static(favlib, oracle, V, maps, n, border):
    """the CPU's warp of that border mode and the model's static masks with it -- once per size and border mode"""
    key = (n, border)
    if key not in _CPU_MASKS:
        cpu_warp = V.warp if border == favlib.BORDER_STN else (lambda img, mp: oracle.warp(img, mp, "cpu"))
        _CPU_MASKS[key] = (cpu_warp, M.static_masks(cpu_warp, maps))
    return _CPU_MASKS[key]


def _cert_oracle(favlib, V, masks, n, case):
    """vr_oracle's VRStylizer for the certainty plane; its static masks are the reference border's, so under the CPU border it is handed
    the masks of that border (the model's, made with the library's warp operator)"""
    ref = _oracle(V, n, case.r, case.inconsistent, case.inconsistent_border)
    if case.border != favlib.BORDER_STN:
        ref = copy.copy(ref)
        ref.mask_left, ref.mask_right, ref.mask_top, ref.mask_bottom = (masks[k][None] for k in (M.L, M.R, M.T, M.B))
    return ref


@functools.lru_cache(maxsize=None)
def _values(n):
    return M.face_values(n, 21)


class Case:
    """one face of one configuration: the inputs, and the handle prepared for it"""

    def __init__(self, favlib, cuda, net, n, mode, i, fill_random=False, seed=1, r=7, border=None, inconsistent=False,
                 inconsistent_border=False, route="file", raw=None):
        self.favlib, self.cuda, self.n, self.mode, self.i, self.route = favlib, cuda, n, mode, i, route
        self.fill_random, self.seed, self.r = fill_random, seed, r
        self.border = favlib.BORDER_STN if border is None else border
        self.inconsistent, self.inconsistent_border = inconsistent, inconsistent_border
        self.single = (i % 6 == 1) if inconsistent else (i == 1)
        self.temporal = i >= 7 and not inconsistent
        self.raw, self.blended = _values(n)
        if raw is not None:
            self.raw = raw
        if route == "file":
            self.frame, self.bw, self.fw = M.frame_u8(n, 100 + i), M.fringe_flow(n, n, 200 + i), None
            self.grey = M.grey_certainty(n, n, 300 + i)
        else:                     # the inputs of tests/test_gpu_vr_post.py's face_flow runs: masks between 10 % and 90 % reliable
            _, self.frame, self.bw, self.fw = VI.face_inputs(n, n)[i - 1]
            self.grey = None
        self.vr = favlib.VR(net, n, n, overlap_w=OV, overlap_h=OV, min_filter_r=r, median=3, fill_random=fill_random, seed=seed,
                            create_inconsistent=inconsistent, create_inconsistent_border=inconsistent_border, border=self.border)

    def prepare(self):
        for k in range(6):
            self.vr.set(1, k, T(self.blended[k], self.cuda))
        for k in range(self.mode):
            self.vr.set(0, k, T(self.raw[k], self.cuda))

    def face(self):
        c, vr = self.cuda, self.vr
        if self.route == "file":
            vr.face(self.i, T(self.frame, c), T(self.bw, c), T(self.grey, c))
        else:
            vr.face_flow(self.i, T(self.frame, c), T(self.bw, c), T(self.fw, c), self.route == "flow4")
        if self.single:
            return None, None, None, vr.last_padded_input().cpu().numpy()
        return vr.get(5).cpu().numpy(), vr.get(6).cpu().numpy(), vr.get(7).cpu().numpy(), vr.last_padded_input().cpu().numpy()

    def dirty(self):
        """another face of another mode with other contents, then fav_vr_finish_frame: tmp_rot, tmp_warp, border, lfw, prior, the
        certainty planes and the input buffer all hold something else afterwards"""
        c, vr, n = self.cuda, self.vr, self.n
        for k in range(6):
            vr.set(0, k, T(self.blended[5 - k] * F(0.5), c))
        other = 7 + ((self.mode + 3) % 6 or 2)        # (never mode 0: under -create_inconsistent that face is a single image)
        vr.face(other, T(M.frame_u8(n, 900), c), T(M.fringe_flow(n, n, 901), c), T(M.grey_certainty(n, n, 902), c))
        vr.finish_frame(want_equi=False, want_cube=False)


TALLY = {"certainty": 0, "border": 0, "prior": 0, "input": 0}


def _check(case, oracle, V):
    """the four tensors of one case against the model, and their bits once more after the buffers were dirtied; returns them"""
    favlib, n, mode, i = case.favlib, case.n, case.mode, case.i
    maps, warp, masks, grads = _static(favlib, V, case.cuda, n, case.border)
    tag = f"{n}x{n} face {i} (mode {mode}) {case.route} fill {int(case.fill_random)}/{case.seed} r {case.r} border {case.border}"
    case.prepare()
    cert, b, p, x = case.face()
    pad = 16
    assert x.shape == (n + 2 * pad, n + 2 * pad, 8)
    if case.single:
        for kind, msg in ((6, MSG6), (7, MSG7)):
            with pytest.raises(favlib.FavError, match=msg):
                case.vr.get(kind)
        want_x = M.padded_input(case.frame, None, None, case.fill_random, case.seed, i, pad)
    else:
        stn = case.border == favlib.BORDER_STN
        ref = _oracle(V, n, case.r, case.inconsistent, case.inconsistent_border)
        # ---- certainty: vr_oracle's plane
        cert01 = None
        if case.temporal:
            if case.route == "file":
                cert01 = case.grey.astype(F) / F(255)
            else:
                mask = oracle.consistency(case.bw, case.fw, case.frame if case.route == "flow4" else None)
                assert 0.10 <= VI.reliable_fraction(mask) <= 0.90
                assert np.array_equal(case.vr.last_mask().cpu().numpy(), mask), f"{tag}: mask"
                cert01 = mask.astype(F) / F(255)
        want_c = _cert_oracle(favlib, V, masks, n, case)._cert(i, mode, cert01)[0]
        assert np.array_equal(cert, want_c), f"{tag}: certainty plane, {int((cert != want_c).sum())} of {cert.size} values differ"
        TALLY["certainty"] += cert.size
        # ---- border
        want_b = M.border(mode, case.raw, warp, maps, masks["all_div"], case.inconsistent_border)
        assert np.array_equal(b, want_b), f"{tag}: border sum, {int((b != want_b).sum())} of {b.size} values differ"
        if mode == 0 or case.inconsistent_border:
            assert not b.any()
        else:
            assert np.abs(b).max() > 0.5
        # ---- prior, on the GPU's own border and certainty
        lfw = warp(case.blended[mode], np.stack([case.bw[..., 1], case.bw[..., 0]])) if case.temporal else None
        want_p = M.prior(mode, case.temporal, lfw, b, cert, grads, masks)
        assert np.array_equal(p, want_p), f"{tag}: prior, {int((p != want_p).sum())} of {p.size} values differ"
        # ---- both against the CPU alone
        scale = max(1.0, max(float(np.abs(a).max()) for a in list(case.raw) + list(case.blended)))
        cpu_warp, cpu_masks = _cpu_static(favlib, oracle, V, maps, n, case.border)
        cpu_b = M.border(mode, case.raw, cpu_warp, maps, cpu_masks["all_div"], case.inconsistent_border)
        cpu_lfw = cpu_warp(case.blended[mode], oracle.flo_to_lua(case.bw)) if case.temporal else None
        cpu_p = M.prior(mode, case.temporal, cpu_lfw, cpu_b, cert, grads, cpu_masks)
        if stn:                  # ... which under the reference's border is vr_oracle's own _prior
            ref.last, ref.prev = list(case.raw), list(case.blended)
            assert np.array_equal(cpu_b, ref._prior(mode + 1, mode, cert[None], None)) and np.array_equal(cpu_p, ref._prior(i, mode, cert[None], case.bw))
        e_b, e_p = float(np.abs(b - cpu_b).max()), float(np.abs(p - cpu_p).max())
        print(f"VR input {tag}: border and prior against the CPU alone: max-abs {e_b:.3e}, {e_p:.3e} (bound {TOL * scale:.3e})")
        assert e_b <= TOL * scale and e_p <= TOL * scale, tag
        TALLY["border"] += b.size; TALLY["prior"] += p.size
        want_x = M.padded_input(case.frame, p, cert, case.fill_random, case.seed, i, pad)
    assert np.array_equal(x, want_x), f"{tag}: padded input, {int((x != want_x).sum())} of {x.size} values differ"
    TALLY["input"] += x.size
    case.dirty()
    case.prepare()
    again = case.face()
    for name, a, g in zip(("certainty", "border", "prior", "input"), (cert, b, p, x), again):
        if a is not None:
            assert np.array_equal(a.view(np.uint32), g.view(np.uint32)), f"{tag}: {name} after the buffers were dirtied: other bits"
    print("VR input values compared so far, none different: " + ", ".join(f"{k} {v}" for k, v in TALLY.items()))
    return cert, b, p, x


def _frames(mode):
    return (mode + 1, 7 + mode, 19 + mode)          # frame 1: not temporal; frames 2 and 4: temporal, two indices of the fill


def _configs(favlib):
    return {"vgg-mean-r7-stn": dict(fill_random=False, seed=1, r=7, border=favlib.BORDER_STN),
            "random5-r7-cpu": dict(fill_random=True, seed=5, r=7, border=favlib.BORDER_CPU),
            "random6-r1-stn": dict(fill_random=True, seed=6, r=1, border=favlib.BORDER_STN),
            "vgg-mean-r1-cpu": dict(fill_random=False, seed=1, r=1, border=favlib.BORDER_CPU)}


@pytest.mark.parametrize("mode", range(6))
@pytest.mark.parametrize("cfg", ["vgg-mean-r7-stn", "random5-r7-cpu", "random6-r1-stn", "vgg-mean-r1-cpu"])
def test_face_input_64(favlib, oracle, V, cuda, net, cfg, mode):
    for i in _frames(mode):
        _check(Case(favlib, cuda, net, 64, mode, i, **_configs(favlib)[cfg]), oracle, V)


@pytest.mark.parametrize("mode", range(6))
@pytest.mark.parametrize("cfg", ["vgg-mean-r7-stn", "random5-r7-cpu", "random6-r1-stn"])
def test_face_input_260(favlib, oracle, V, cuda, net, cfg, mode):
    """rotate_kernel's second block (ragged), accum / prior kernels over 264 blocks, padded rows of 292"""
    for i in _frames(mode):
        _check(Case(favlib, cuda, net, 260, mode, i, **_configs(favlib)[cfg]), oracle, V)


@pytest.mark.parametrize("fill_random", [False, True], ids=["vgg-mean", "uniform-random"])
def test_create_inconsistent_64(favlib, oracle, V, cuda, net, fill_random):
    """every i % 6 == 1 is a single image (fast_artistic_video_vr.lua:304-310), nothing is temporal"""
    for i in (1, 2, 3, 4, 5, 6, 7, 8, 12, 13):
        c = Case(favlib, cuda, net, 64, (i - 1) % 6, i, fill_random=fill_random, seed=9, inconsistent=True)
        assert c.single == (i in (1, 7, 13)) and not c.temporal
        _, b, p, _ = _check(c, oracle, V)
        if not c.single:
            assert np.array_equal(b, p)          # the prior is the border sum, whatever the frame


def test_create_inconsistent_border_64(favlib, oracle, V, cuda, net):
    """the border is zero (the hipMemsetAsync branch), no border mask enters the certainty, the raw faces of the frame are not needed.
    The rerun of every case finds the border buffer full of fav_vr_finish_frame's last sum: only the memset makes it zero again."""
    for mode in range(6):
        for i in (mode + 1, 7 + mode):
            c = Case(favlib, cuda, net, 64, mode, i, fill_random=True, seed=3, inconsistent_border=True)
            c.prepare = lambda c=c: [c.vr.set(1, k, T(c.blended[k], cuda)) for k in range(6)]      # no raw face at all
            cert, b, p, _ = _check(c, oracle, V)
            if not c.single:
                assert not b.any()
                if not c.temporal:
                    assert not cert.any() and not p.any()


@pytest.mark.parametrize("route", ["flow3", "flow4"])
@pytest.mark.parametrize("mode", [1, 5])
def test_face_flow_input_260(favlib, oracle, V, cuda, net, mode, route):
    """the certainty from the two flows (fav_vr_face_flow, the checker's 3- and 4-argument mode) instead of a file's bytes"""
    _check(Case(favlib, cuda, net, 260, mode, 7 + mode, fill_random=True, seed=7, route=route), oracle, V)


def test_sphere_border_64(favlib, oracle, V, cuda, net):
    """tests/test_cpu_vr_input.py::test_sphere_border_per_mode on the GPU's border: six faces of ONE image of the sphere, so the border
    of a face is the face's own content x the mask sum / the divisor -- a check that rests on no restatement's neighbour table.
    Bound: M.SPHERE_BOUND, twice the model's own deviation (M.SPHERE_MEASURED, recorded there)."""
    maps, warp, masks, _ = _static(favlib, V, cuda, 64, favlib.BORDER_STN)
    faces = M.sphere_faces()
    for mode in range(1, 6):
        c = Case(favlib, cuda, net, 64, mode, mode + 1, raw=faces)
        c.prepare()
        _, b, _, _ = c.face()
        want, where = M.sphere_expected(mode, faces, masks)
        e = float(np.abs(b.astype(np.float64) - want)[:, where].max())
        print(f"VR input sphere faces, mode {mode}: worst |border - expected| {e:.6e} (bound {M.SPHERE_BOUND[mode]:.6e})")
        assert e <= M.SPHERE_BOUND[mode], mode


def test_refusals_write_nothing(favlib, cuda, net):
    import torch
    n = 64
    raw, blended = _values(n)
    vr = favlib.VR(net, n, n, overlap_w=OV, overlap_h=OV, median=3)
    face_buf = torch.full((3, n, n), 0.25, dtype=torch.float32, device=cuda)
    pad_buf = torch.full((n + 32, n + 32, 8), 0.25, dtype=torch.float32, device=cuda)

    def refused(kind, msg):
        with pytest.raises(favlib.FavError, match=msg):
            vr.get(kind, out=face_buf)
        assert (face_buf.cpu().numpy() == 0.25).all()

    frame = T(M.frame_u8(n, 1), cuda)
    # a fresh handle: nothing of any of the three
    refused(6, MSG6); refused(7, MSG7)
    with pytest.raises(favlib.FavError, match=MSGP):
        vr.last_padded_input(pad_buf)
    assert (pad_buf.cpu().numpy() == 0.25).all()
    with pytest.raises(favlib.FavError, match="libfav error -1: fav_vr_get_padded_input_f32: null pointer"):
        favlib._check(favlib.lib().fav_vr_get_padded_input_f32(vr.h, None, None))
    # a single image: an input, but neither a border nor a prior
    vr.face(1, frame)
    refused(6, MSG6); refused(7, MSG7)
    assert vr.last_padded_input().cpu().numpy()[..., :3].std() > 1
    # a face with a prior: all three; fav_vr_finish_frame reuses the border buffer, and this face's prior was the border
    vr.face(2, frame)
    assert np.array_equal(vr.get(6).cpu().numpy(), vr.get(7).cpu().numpy()) and vr.get(6).cpu().numpy().any()
    for k in range(2, 6):
        vr.set(0, k, T(raw[k], cuda))
    vr.finish_frame(want_equi=False, want_cube=False)
    refused(6, MSG6); refused(7, MSG7)
    kept = vr.last_padded_input().cpu().numpy()
    # a temporal face's prior lies in a buffer of its own: it outlives fav_vr_finish_frame, the border sum does not
    for k in range(6):
        vr.set(0, k, T(raw[k], cuda))
    vr.face(12, frame, T(M.fringe_flow(n, n, 2), cuda), T(M.grey_certainty(n, n, 3), cuda))
    assert not np.array_equal(vr.last_padded_input().cpu().numpy(), kept)
    p = vr.get(7).cpu().numpy()
    assert not np.array_equal(p, vr.get(6).cpu().numpy())
    vr.finish_frame(want_equi=False, want_cube=False)
    refused(6, MSG6)
    assert np.array_equal(vr.get(7).cpu().numpy(), p)
    # kinds that do not exist are still refused by their number
    with pytest.raises(favlib.FavError, match="fav_vr_get_f32: nothing of kind 8"):
        favlib._check(favlib.lib().fav_vr_get_f32(vr.h, 8, 0, favlib._p(face_buf), favlib._stream()))
    assert (face_buf.cpu().numpy() == 0.25).all()
    with pytest.raises(favlib.FavError, match="VR.get: out must be"):
        vr.get(6, out=pad_buf)
    # a single image after a face with a prior: both are refused again
    vr.face(1, frame)
    refused(6, MSG6); refused(7, MSG7)
