"""What a cube face's network reads, on the CPU: tests/util/vr_input_model.py (written from the reference's Lua) against
oracle/vr_oracle.py's VRStylizer (the other restatement) -- EQUAL in every mode -- and against a check that rests on neither one's
neighbour table: six faces cut from ONE image of the sphere.  No GPU.  tests/test_gpu_vr_input.py holds the library to the same model.

fav_vr_map_host's four perspective maps are held EQUAL to vr_oracle's by tests/test_cpu_oracle.py::test_vr_static_maps_host_vs_oracle;
the static masks are warps of ones through those maps on the device and are compared in tests/test_gpu_vr_input.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import vr_input_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N, OV = 64, 24


@pytest.fixture(scope="module")
def V(oracle):
    import vr_oracle
    return vr_oracle


@pytest.fixture(scope="module")
def static(V):
    """maps, masks and gradient masks of the model at 64x64, overlap 24, with the CPU warp"""
    maps = {M.L: V.warp_map_left(N, OV, N), M.R: V.warp_map_right(N, OV, N), M.T: V.warp_map_top(N, OV, N), M.B: V.warp_map_bottom(N, OV, N)}
    return maps, M.static_masks(V.warp, maps), M.grad_masks(N, N, OV, OV)


def test_static_masks_and_gradient_masks_equal_the_oracle(V, static):
    maps, masks, grads = static
    ref = V.VRStylizer(None, N, N, overlap_w=OV, overlap_h=OV)
    for k, want in ((M.L, ref.mask_left), (M.R, ref.mask_right), (M.T, ref.mask_top), (M.B, ref.mask_bottom), ("all", ref.mask_all),
                    ("all_div", ref.mask_all_div)):
        assert np.array_equal(masks[k], want[0]), k
    for k, want in ((M.L, ref.g_left), (M.R, ref.g_right), ("left_right", ref.g_lr), ("all", ref.g_all)):
        assert np.array_equal(grads[k], want[0].astype(F)), k
    assert 0 < masks[M.L].mean() < 1 and masks["all_div"].max() > 1


def test_rotations_are_the_reference_s(V):
    a = np.random.default_rng(0).random((3, 5, 7)).astype(F)
    assert np.array_equal(M.rotate(a, M.ROT90), V.rotate90(a)) and np.array_equal(M.rotate(a, M.ROTM90), V.rotate_minus90(a))
    assert np.array_equal(M.rotate(a, M.ROT180), V.rotate180(a)) and M.rotate(a, M.ROT0) is a
    # fast_artistic_video_vr.lua:134-136 spelled out: transpose, then reverse the rows
    assert np.array_equal(M.rotate(a, M.ROT90), np.transpose(a, (0, 2, 1))[:, ::-1]) and M.rotate(a, M.ROT90).shape == (3, 7, 5)


def test_inputs_are_what_the_tests_need():
    g = M.grey_certainty(N, N, 5)
    assert set(np.unique(g)) == set(range(256))
    bw = M.fringe_flow(N, N, 6)
    yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    out = (xx + bw[..., 0] < 0) | (xx + bw[..., 0] > N - 1) | (yy + bw[..., 1] < 0) | (yy + bw[..., 1] > N - 1)
    assert 0.02 < out.mean() < 0.3 and 1 < np.abs(bw).max() < 8
    assert not np.array_equal(bw * 8, np.round(bw * 8))
    M.face_values(N, 7)


CASES = [(mode, i) for mode in range(6) for i in (mode + 1, 7 + mode, 19 + mode)]


@pytest.mark.parametrize("opts", [dict(), dict(create_inconsistent=True), dict(create_inconsistent_border=True)],
                         ids=["plain", "create_inconsistent", "create_inconsistent_border"])
@pytest.mark.parametrize("fill_random,seed,r", [(False, 1, 7), (True, 5, 7), (True, 6, 1)], ids=["vgg-mean-r7", "random5-r7", "random6-r1"])
def test_model_equals_vr_oracle(V, oracle, static, monkeypatch, opts, fill_random, seed, r):
    """3(a): border, prior and the un-padded input of the model are EQUAL to VRStylizer._prior / _fill / the x of face(), every mode,
    temporal and not"""
    maps, masks, grads = static
    raw, blended = M.face_values(N, 21)
    seen = {}
    monkeypatch.setattr(V.O, "net_forward", lambda layers, x, *a, **k: seen.setdefault("x", np.array(x)) [:3])
    compared = 0
    for mode, i in CASES:
        frame = M.frame_u8(N, 100 + i)
        bw = M.fringe_flow(N, N, 200 + i)
        grey = M.grey_certainty(N, N, 300 + i)
        ref = V.VRStylizer(None, N, N, overlap_w=OV, overlap_h=OV, min_filter_r=r, fill_random=fill_random, seed=seed, **opts)
        ref.last = [raw[k] if k < mode else None for k in range(6)]
        ref.prev = list(blended)
        ref._finish = lambda: None
        single = (i % 6 == 1) if opts.get("create_inconsistent") else (i == 1)
        temporal = i >= 7 and not opts.get("create_inconsistent")
        cert01 = grey.astype(F) / F(255)
        seen.clear()
        ref.face(i, M.f01(frame), bw, cert01)
        x = seen["x"]
        if single:
            got = M.padded_input(frame, None, None, fill_random, seed, i, 0)
        else:
            cert = ref._cert(i, mode, cert01)[0]
            b = M.border(mode, ref.last, V.warp, maps, masks["all_div"], bool(opts.get("create_inconsistent_border")))
            lfw = V.warp(blended[mode], oracle.flo_to_lua(bw)) if temporal else None
            p = M.prior(mode, temporal, lfw, b, cert, grads, masks)
            want_p = ref._prior(i, mode, cert[None], bw)
            assert np.array_equal(p, want_p), f"prior of face {i} (mode {mode}): {int((p != want_p).sum())} values differ"
            if not temporal:
                assert np.array_equal(b, want_p)
            if mode == 0 or opts.get("create_inconsistent_border"):
                assert not b.any()
            else:
                assert np.abs(b).max() > 0.5
            got = M.padded_input(frame, p, cert, fill_random, seed, i, 0)
            if fill_random:
                assert np.array_equal(np.transpose(got[..., 3:6], (2, 0, 1)), ref._fill(i, cert[None]) + oracle.preprocess(p) * cert[None])
            compared += 1
        assert got.shape == (N, N, 8) and not got[..., 7].any()
        assert np.array_equal(np.transpose(got[..., :7], (2, 0, 1)), x), f"input of face {i} (mode {mode}): {int((np.transpose(got[..., :7], (2, 0, 1)) != x).sum())} values differ"
    assert compared >= (12 if opts.get("create_inconsistent") else 17)


def test_padding_is_a_reflection_without_edge_repeat():
    assert list(M.reflect(5, 3)) == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    frame = M.frame_u8(8, 1)
    p = M.padded_input(frame, None, None, True, 3, 4, 3)
    core = M.padded_input(frame, None, None, True, 3, 4, 0)
    assert p.shape == (14, 14, 8) and np.array_equal(p[3:-3, 3:-3], core)
    assert np.array_equal(p[0, 3:-3], core[3]) and np.array_equal(p[-1, 3:-3], core[4]) and np.array_equal(p[3:-3, -1], core[:, 4])
    assert not np.array_equal(core, M.padded_input(frame, None, None, True, 3, 5, 0))         # the fill is keyed by the face index


def test_fill_differs_between_frames_and_seeds():
    """the premise of "a wrong RNG index shows" in tests/test_gpu_vr_input.py: the fill of face 8 is neither face 20's, nor face 2's,
    nor another seed's"""
    xs = [M.padded_input(M.frame_u8(64, 1), None, None, True, s, i, 0)[..., 3:6] for s, i in ((5, 8), (5, 20), (6, 8), (5, 2))]
    assert all(not np.array_equal(xs[0], o) and np.abs(xs[0] - o).mean() > 10 for o in xs[1:])


# ------------------------------------------------------------------------------------------------ 3(c) one sphere, six faces
def _deviation(mode, faces, V, static, table=None):
    maps, masks, _ = static
    want, where = M.sphere_expected(mode, faces, masks)
    got = M.border(mode, faces, V.warp, maps, masks["all_div"], False, table)
    assert where.any()
    return float(np.abs(got.astype(np.float64) - want)[:, where].max())


@pytest.fixture(scope="module")
def sphere():
    return M.sphere_faces()


def test_sphere_border_per_mode(V, static, sphere):
    """Every border pixel shows the piece of the sphere the face shows there itself: border == own content x (sum of the warped-ones
    masks of the mode's terms) / the mode's divisor, up to what the perspective maps and the bilinear taps leave on a smooth image.
    Measured with vr_oracle.warp at 64x64, overlap 24, over the pixels whose mask sum is positive (0..1 images), worst per mode:
        mode 1  1.349932e-02    mode 2  1.384741e-02    mode 3  1.515853e-02    mode 4  1.538138e-02    mode 5  1.399371e-02
    (M.SPHERE_MEASURED).  The bound is twice that: the margin covers nothing but the size dependence of bilinear error.
    The least visible of the 132 single-entry changes of the table (next test) is 10.5 times the bound."""
    for mode in range(1, 6):
        e = _deviation(mode, sphere, V, static)
        print(f"sphere faces, mode {mode}: worst |border - expected| {e:.6e} (recorded {M.SPHERE_MEASURED[mode]:.6e}, bound {M.SPHERE_BOUND[mode]:.6e})")
    for mode in range(1, 6):
        assert _deviation(mode, sphere, V, static) <= M.SPHERE_BOUND[mode], mode


def test_every_single_entry_change_of_the_table_is_caught(V, static, sphere):
    """the test of the test: one entry of the table changed at a time -- each rotation to each other rotation, each map to each other
    map, each source face to each other face -- exceeds TEN times the bound"""
    n, worst = 0, None
    for mode in range(1, 6):
        for what, table in M.table_changes(mode):
            e = _deviation(mode, sphere, V, static, table)
            ratio = e / M.SPHERE_BOUND[mode]
            if worst is None or ratio < worst[0]:
                worst = (ratio, what, e)
            assert e > 10 * M.SPHERE_BOUND[mode], f"{what}: deviation {e:.4e} is not above ten times the bound {M.SPHERE_BOUND[mode]:.4e}"
            n += 1
    print(f"{n} single-entry changes of the table; the least visible: {worst[1]}, deviation {worst[2]:.4e} = {worst[0]:.1f} x the bound")
    assert n == 12 * 11


# ------------------------------------------------------------------------------------------------ symbols and binding
def test_fav_vr_state_h_is_exported_and_bound(favlib):
    hdr = open(os.path.join(ROOT, "include", "fav_vr_state.h")).read()
    declared = set(re.findall(r"^int (fav_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == {"fav_vr_set_f32", "fav_vr_get_padded_input_f32"} == set(favlib.EXPORTS_VR_STATE)
    out = subprocess.run(["nm", "-D", "--defined-only", favlib.LIB_PATH], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in declared:
        assert name in defined and name not in favlib.EXPORTS
        getattr(favlib.lib(), name)
    L = favlib.lib()
    assert L.fav_vr_get_padded_input_f32(None, None, None) == -1 and b"fav_vr_get_padded_input_f32: null handle" in L.fav_last_error()
    assert callable(favlib.VR.last_padded_input)
