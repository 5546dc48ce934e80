"""The 360-degree post-processing (fav_vr_finish_frame: post-blend, median3_kernel / median_kernel, rotate_kernel, strip_kernel, the
equirectangular warp, the u8 quantisation) on faces the TEST chooses (fav_vr_set_f32, include/fav_vr_state.h), at sizes with more than
one 256-lane block per row, held to tests/util/vr_post_model.py -- bit for bit where the operation is a selection, a copy or one rounding.

Per case (six faces set, finish_frame):
  blended faces  get(1, k)  within 1e-5 of oracle/vr_oracle.py's _finish on the same faces (they contain the warp, which the project
                            holds to 1e-5); non-finite values in the same places
  filtered faces get(2, k)  EQUAL to the model's median of the GPU's own blended faces (windows that hold a NaN left out)
  cube-map strip get(4)     EQUAL to the model's strip of the GPU's own filtered faces; for coded faces every pixel of the un-blended
                            interior is decoded and its source face, row and column asserted from the definition alone
  equirectangular get(3)    within 1e-5 of the oracle's warp of the model's input strip of the GPU's own filtered faces
  both u8 images            EQUAL to the model's quantisation of the GPU's own float images; written completely (0x00- and 0xFF-filled
                            output buffers give the same bytes)
-0.0 and +0.0 compare equal (np.array_equal on values): fminf(-0, +0) may return either.

Sizes: 260 (two blocks per row, the second ragged; the r = 3 median writes 258 columns, the r = 5 median exactly 256), 516 (three
blocks; the oracle's _finish takes about 1 s there with r = 3 and 2.5 s with r = 5 on 16 CPU threads, so 388 was not needed), 64 for
the sweep of median x overlaps x equirectangular output.  Contents: tests/util/vr_post_model.py faces()."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import vr_check_inputs as VI  # noqa: E402
import vr_post_model as M  # noqa: E402

from fav_amd import t7  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 1e-5
SQUARE_MSG = "the cube-map strip needs square cropped faces"


def T(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev) if a is not None else None      # (a copy: the shared faces are read-only)


@pytest.fixture(scope="module")
def net(favlib, golden_dir):
    return favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)


@pytest.fixture(scope="module")
def V(oracle):
    import vr_oracle
    return vr_oracle


@functools.lru_cache(maxsize=None)
def _faces(n, variant):
    fs = M.faces(n, variant)
    for f in fs:
        f.setflags(write=False)
    return fs


def _oracle_finish(V, n, variant, kw):
    """VRStylizer._finish on the faces; with crops that are not square it stops at the cube map, everything before it is there"""
    chk = V.VRStylizer(None, n, n, overlap_w=kw["overlap_w"], overlap_h=kw["overlap_h"], median=kw["median"],
                       out_equi_w=kw["out_equi_w"], out_equi_h=kw["out_equi_h"])
    chk.last = list(_faces(n, variant))
    try:
        chk._finish()
    except ValueError:
        assert kw["overlap_w"] != kw["overlap_h"] and chk.filtered is not None
    return chk


def _err(got, want):
    """max |got - want| over the finite values of want; the non-finite ones must be the same values in the same places"""
    nf = ~np.isfinite(want)
    assert np.array_equal(nf, ~np.isfinite(got)), "non-finite values in other places than the oracle's"
    assert np.array_equal(got[nf], want[nf], equal_nan=True)
    return float(np.abs(got[~nf].astype(np.float64) - want[~nf]).max())


def _finish_into(favlib, vr, cuda, fill, want_equi, want_cube):
    """fav_vr_finish_frame into buffers pre-filled with `fill`"""
    import torch
    e = torch.full((vr.equi_h, vr.equi_w, 3), fill, dtype=torch.uint8, device=cuda) if want_equi else None
    c = torch.full((vr.cube_h, vr.cube_w, 3), fill, dtype=torch.uint8, device=cuda) if want_cube else None
    favlib._check(favlib.lib().fav_vr_finish_frame(vr.h, favlib._p(e), favlib._p(c), favlib._stream()))
    return (e.cpu().numpy() if want_equi else None), (c.cpu().numpy() if want_cube else None)


def _set_six(vr, faces, cuda):
    for k in range(6):
        vr.set(0, k, T(faces[k], cuda))


def _case(favlib, oracle, V, cuda, net, n, med, ow, oh, equi, variant, nan_cap=False):
    import torch
    kw = dict(overlap_w=ow, overlap_h=oh, median=med, out_equi_w=equi[0], out_equi_h=equi[1])
    faces = _faces(n, variant)
    chk = _oracle_finish(V, n, variant, kw)
    r = med // 2
    tag = f"{n}x{n} median {med} overlap {ow}/{oh} equi {equi[0]}x{equi[1]} {variant}"
    left_out = 0
    if nan_cap:      # a condition on the model alone, before the GPU's result is looked at
        per_plane = np.array([M.nan_windows(b, med).sum(axis=(1, 2)) for b in chk.blended])
        left_out = int(per_plane.max())
        assert left_out <= M.NAN_PER_FACE * med * med and left_out < 0.01 * (n - med + 1) ** 2, (left_out, tag)
    else:
        assert not any(np.isnan(b).any() for b in chk.blended)

    vr = favlib.VR(net, n, n, **kw)
    assert (vr.filt_h, vr.filt_w) == (n - 2 * r, n - 2 * r) and (vr.equi_w, vr.equi_h) == equi
    square = ow == oh
    ovh, ovw, ch, cw = M.cube_crop(n, n, ow, oh, med)
    assert (vr.cube_h, vr.cube_w) == ((ch, 6 * cw) if square else (0, 0))
    _set_six(vr, faces, cuda)
    if not square:
        # fav_vr_create accepts the handle (no cube-map strip: cube_w = 0); it is fav_vr_finish_frame that refuses a cube-map buffer
        dummy = torch.zeros(16, dtype=torch.uint8, device=cuda)
        with pytest.raises(favlib.FavError, match="libfav error -1: fav_vr_finish_frame: " + SQUARE_MSG):
            favlib._check(favlib.lib().fav_vr_finish_frame(vr.h, None, favlib._p(dummy), favlib._stream()))
        assert (dummy.cpu().numpy() == 0).all()
        _set_six(vr, faces, cuda)               # (the refused call had blended and filtered already: the frame's faces are spent)
    want_equi = equi[0] > 0
    e8, c8 = _finish_into(favlib, vr, cuda, 0x00, want_equi, square)

    blend = [vr.get(1, k).cpu().numpy() for k in range(6)]
    filt = [vr.get(2, k).cpu().numpy() for k in range(6)]
    e_blend = max(_err(blend[k], chk.blended[k]) for k in range(6))
    # ---- median: a selection, exact
    for k in range(6):
        want = M.median(blend[k], med)
        keep = ~M.nan_windows(blend[k], med)
        assert filt[k].shape == want.shape
        assert np.array_equal(filt[k][keep], want[keep]), f"{tag}: median-filtered face {k}: {int((filt[k][keep] != want[keep]).sum())} values differ"
        if nan_cap:
            assert (~keep).sum(axis=(1, 2)).max() == left_out
            assert np.array_equal(np.isnan(filt[k][keep]), np.zeros(int(keep.sum()), bool))       # no NaN outside its windows
    # ---- cube-map strip: copies, exact
    if square:
        cube = vr.get(4).cpu().numpy()
        assert np.array_equal(cube, M.cube_strip(filt, n, n, ow, oh, med), equal_nan=True), f"{tag}: cube-map strip"
        ok = ~np.isnan(np.transpose(cube, (1, 2, 0)))
        assert np.array_equal(c8[ok], M.quantize(cube)[ok]), f"{tag}: cube-map u8"
        if variant in ("coded", "nan"):
            face, yy, xx, interior = M.cube_sources(n, ow, oh, med)
            assert interior.mean() > 0.3
            for c in range(3):
                fk, fy, fx = M.decode(cube[c], c)
                # a window that holds a NaN of the RAW face returns something unspecified (not always NaN): left out, on the model alone
                nanw = np.stack([np.pad(M.nan_windows(faces[k][c:c + 1], med)[0], r) for k in range(6)])
                sel = interior & ~nanw[face, yy, xx]
                assert sel.sum() >= interior.sum() - M.NAN_PER_FACE * 6 * max(med, 1) ** 2
                assert np.array_equal(fk[sel], face[sel]) and np.array_equal(fy[sel], yy[sel]) and np.array_equal(fx[sel], xx[sel]), \
                    f"{tag}: cube-map strip shows another source pixel (channel {c})"
    else:
        with pytest.raises(favlib.FavError, match="fav_vr_get_f32"):
            vr.get(4)
    # ---- equirectangular image
    e_equi = 0.0
    if want_equi:
        eq = vr.get(3).cpu().numpy()
        e_equi = _err(eq, V.warp(M.equi_strip(filt), chk.equi_map))
        ok = ~np.isnan(np.transpose(eq, (1, 2, 0)))
        assert np.array_equal(e8[ok], M.quantize(eq)[ok]), f"{tag}: equirectangular u8"
    else:
        with pytest.raises(favlib.FavError, match="fav_vr_get_f32"):
            vr.get(3)
        _set_six(vr, faces, cuda)
        dummy = torch.zeros(16, dtype=torch.uint8, device=cuda)
        with pytest.raises(favlib.FavError, match="created without an equirectangular output size"):
            favlib._check(favlib.lib().fav_vr_finish_frame(vr.h, favlib._p(dummy), None, favlib._stream()))
    print(f"VR post {tag}: blended max-abs {e_blend:.3e}, equirectangular {e_equi:.3e} (bound {TOL:g})"
          + (f", NaN windows left out per plane {left_out} (cap {M.NAN_PER_FACE * med * med})" if nan_cap else ""))
    assert e_blend <= TOL and e_equi <= TOL, (tag, e_blend, e_equi)
    # ---- the same frame again into 0xFF-filled buffers: every byte is written
    _set_six(vr, faces, cuda)
    e8b, c8b = _finish_into(favlib, vr, cuda, 0xFF, want_equi, square)
    if want_equi:
        assert np.array_equal(e8, e8b)
    if square:
        assert np.array_equal(c8, c8b)
    return vr, blend, filt


CASES_260 = [(m, v) for m in (0, 3, 5) for v in ("coded", "ties")] + [(3, "inf"), (5, "inf"), (0, "range"), (3, "range")]


@pytest.mark.parametrize("med,variant", CASES_260, ids=[f"median{m}-{v}" for m, v in CASES_260])
def test_finish_frame_260(favlib, oracle, V, cuda, net, med, variant):
    """two blocks per row, the second ragged (r = 3: 258 filtered columns; r = 5: exactly 256)"""
    _case(favlib, oracle, V, cuda, net, 260, med, 24, 24, (96, 48), variant)


@pytest.mark.parametrize("med,variant", [(3, "coded"), (5, "ties"), (0, "coded")], ids=["median3-coded", "median5-ties", "median0-coded"])
def test_finish_frame_516(favlib, oracle, V, cuda, net, med, variant):
    """three blocks per row"""
    _case(favlib, oracle, V, cuda, net, 516, med, 24, 24, (96, 48), variant)


@pytest.mark.parametrize("equi", [(96, 48), (0, 0)], ids=["equi96x48", "noequi"])
@pytest.mark.parametrize("ow,oh", [(24, 24), (12, 40), (40, 12)])
@pytest.mark.parametrize("med", [0, 3, 5])
def test_finish_frame_option_sweep_64(favlib, oracle, V, cuda, net, med, ow, oh, equi):
    """asymmetric overlaps on a square face give crops that are not square: fav_vr_create accepts them without a cube-map strip,
    fav_vr_finish_frame refuses a cube-map buffer with its message, and the equirectangular output is still exact"""
    _case(favlib, oracle, V, cuda, net, 64, med, ow, oh, equi, "ties" if med else "coded")


@pytest.mark.parametrize("med", [3, 5])
def test_nan_stays_inside_its_windows(favlib, oracle, V, cuda, net, med):
    """20 isolated NaNs per face.  What a window that holds a NaN returns is unspecified (utils.lua:157 does not define it) and
    differs between the two kernels -- printed here; every other value of every output is still exact."""
    vr, blend, filt = _case(favlib, oracle, V, cuda, net, 260, med, 24, 24, (96, 48), "nan", nan_cap=True)
    w = M.nan_windows(blend[0], med)
    got = filt[0][w]
    print(f"VR post NaN windows, r = {med}: {int(np.isnan(got).sum())} of {got.size} return NaN, the others a finite value of the window")
    assert w.sum() == 3 * M.NAN_PER_FACE * med * med


# ------------------------------------------------------------------------------------------------ the per-face path beyond one block
def _f01(u8):
    return np.transpose(u8, (2, 0, 1)).astype(F) / F(255)


FACE_PATHS = [("file", False, 0), ("file", True, 0), ("flow", True, 0), ("flow", True, 1)]
FACE_IDS = ["face-vgg-mean", "face-uniform-random", "face_flow-3arg", "face_flow-4arg"]
_RUNS = {}


def _faces_run(favlib, oracle, V, cuda, net, golden_dir, path, fill_random, structure):
    """one frame of six faces and the first two of a second at 260x260, teacher-forced as test_gpu_vr.py::test_vr_two_frames_vs_oracle;
    run once per parameter set: [(i, mode, max-abs of the face, get(5), oracle's plane)]"""
    key = (path, fill_random, structure)
    if key in _RUNS:
        return _RUNS[key]
    n = 260
    layers = t7.extract_layers(t7.load(os.path.join(golden_dir, "tiny_model.t7"))["model"])
    kw = dict(overlap_w=24, overlap_h=24, median=3, seed=7, fill_random=fill_random)
    vr = favlib.VR(net, n, n, **kw)
    rng = np.random.default_rng(11)
    out = []
    for (i, f, bw, fw) in VI.face_inputs(n, n)[:8]:
        mode = (i - 1) % 6
        tf = V.VRStylizer(layers, n, n, **kw)
        for k in range(mode):
            tf.last[k] = vr.get(0, k).cpu().numpy()
        if i >= 7:
            tf.prev = [vr.get(1, k).cpu().numpy() for k in range(6)]
        ce = None
        if i >= 7:
            ce = oracle.consistency(bw, fw, f if structure else None) if path == "flow" else ((rng.random((n, n)) > 0.15) * 255).astype(np.uint8)
        if path == "flow":
            got = vr.face_flow(i, T(f, cuda), T(bw, cuda), T(fw, cuda), structure).cpu().numpy()
            if i >= 7:
                assert 0.10 <= VI.reliable_fraction(ce) <= 0.90
                assert np.array_equal(vr.last_mask().cpu().numpy(), ce), f"mask of face {i}"
        else:
            got = vr.face(i, T(f, cuda), T(bw, cuda), T(ce, cuda)).cpu().numpy()
        cert01 = ce.astype(F) / F(255) if ce is not None else None
        tf._finish = lambda: None
        want = tf.face(i, _f01(f), bw, cert01)
        planes = (None, None)
        if i > 1:
            planes = (vr.get(5).cpu().numpy(), tf._cert(i, mode, cert01)[0])
        out.append((i, mode, float(np.abs(got - want).max())) + planes)
        if mode == 5:
            vr.finish_frame()
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("path,fill_random,structure", FACE_PATHS, ids=FACE_IDS)
def test_faces_260_teacher_forced(favlib, oracle, V, cuda, net, golden_dir, path, fill_random, structure):
    """rotate_kernel's second block, prep_prior_kernel on a padded row wider than 256, vr_check_cert_kernel at W > 256 (whose mask
    must be the oracle's checker's, byte for byte): every face within 2e-4 of the teacher-forced oracle"""
    run = _faces_run(favlib, oracle, V, cuda, net, golden_dir, path, fill_random, structure)
    print(f"VR faces 260x260 {path} fill_random={fill_random} structure={structure}: worst teacher-forced max-abs "
          f"{max(e for (_, _, e, *_) in run):.3e} (bound 2e-4)")
    for (i, mode, e, *_) in run:
        assert e <= 2e-4, f"face {i} (mode {mode}) teacher-forced: {e:.3e}"


@pytest.mark.parametrize("path,fill_random,structure", FACE_PATHS, ids=FACE_IDS)
def test_certainty_plane_260_equals_oracle(favlib, oracle, V, cuda, net, golden_dir, path, fill_random, structure):
    """get(5), the certainty plane after border max and erosion, must EQUAL oracle/vr_oracle.py's: the mask byte / 255, the max with the
    static masks and the erosion are selections.  (While vr_oracle summed its warps in double, rounded once, its static masks -- warps
    of ones -- were one ulp off the reference kernel's fp32 sum in places, and so were 1096 .. 6951 of the 67600 values of these planes,
    max-abs 5.960e-08; it now warps as the reference's kernel does, BilinearSamplerBDHW.cu:103-106, see vr_oracle.warp.)"""
    run = _faces_run(favlib, oracle, V, cuda, net, golden_dir, path, fill_random, structure)
    for (i, mode, _, got, want) in run:
        if got is not None:
            print(f"certainty plane of face {i}: {int((got != want).sum())} of {got.size} values differ from the oracle's")
    for (i, mode, _, got, want) in run:
        if got is not None:
            assert np.array_equal(got, want), f"certainty plane of face {i}: {int((got != want).sum())} values differ from the oracle's"
            assert 0 < got.mean() < 1          # (neither all certain nor all uncertain)


# ------------------------------------------------------------------------------------------------ fav_vr_set_f32 itself
def test_set_refusals(favlib, cuda, net):
    import torch
    n = 64
    vr = favlib.VR(net, n, n, overlap_w=24, overlap_h=24, median=3)
    faces = _faces(n, "coded")
    t = T(faces[0], cuda)
    mark = torch.full((3, n, n), 0.25, dtype=torch.float32, device=cuda)
    for k in range(6):
        vr.set(0, k, mark); vr.set(1, k, mark)
    vr.finish_frame()
    for k in range(6):
        vr.set(0, k, mark)                      # (finish_frame has spent the frame's faces and written the blended ones)
        vr.set(1, k, mark)
    before = [[vr.get(w, k).cpu().numpy() for k in range(6)] for w in (0, 1)]
    for which in (2, 3, 4, 5, -1):
        with pytest.raises(favlib.FavError, match=rf"libfav error -1: fav_vr_set_f32: kind {which} "):
            vr.set(which, 0, t)
    for k in (-1, 6):
        with pytest.raises(favlib.FavError, match=rf"libfav error -1: fav_vr_set_f32: face {k} "):
            vr.set(0, k, t)
    for which in (0, 1):
        with pytest.raises(favlib.FavError, match=r"libfav error -1: fav_vr_set_f32: null pointer"):
            vr.set(which, 0, None)
    with pytest.raises(favlib.FavError, match="contiguous float32"):
        vr.set(0, 0, t[:, :32])
    for w in (0, 1):                             # nothing was written by any of them
        for k in range(6):
            assert np.array_equal(vr.get(w, k).cpu().numpy(), before[w][k])
    fresh = favlib.VR(net, n, n, overlap_w=24, overlap_h=24, median=3)
    for k in range(5):
        fresh.set(0, k, T(faces[k], cuda))
    with pytest.raises(favlib.FavError, match="fav_vr_finish_frame: face 5 of this frame is missing"):
        fresh.finish_frame()
    fresh.set(0, 5, T(faces[5], cuda))
    fresh.finish_frame()
    with pytest.raises(favlib.FavError, match="fav_vr_finish_frame: face 0 of this frame is missing"):
        fresh.finish_frame()                    # the frame's faces are spent


def test_set_blended_faces_resumes_a_run(favlib, cuda, net):
    """which = 1: six blended faces make a previous frame -- face 7 on a fresh handle has the bits of the handle that finished the frame"""
    n = 64
    kw = dict(overlap_w=24, overlap_h=24, median=3, seed=7, fill_random=True)
    a = favlib.VR(net, n, n, **kw)
    _set_six(a, _faces(n, "ties"), cuda)
    a.finish_frame()
    i, f, bw, fw = VI.face_inputs()[6]
    ce = favlib.consistency(T(bw, cuda), T(fw, cuda))
    b = favlib.VR(net, n, n, **kw)
    for k in range(6):
        if k == 5:
            with pytest.raises(favlib.FavError, match="face 7 needs the flow, the certainty and a finished previous frame"):
                b.face(7, T(f, cuda), T(bw, cuda), ce)
        b.set(1, k, a.get(1, k))
    want = a.face(7, T(f, cuda), T(bw, cuda), ce).cpu().numpy()
    got = b.face(7, T(f, cuda), T(bw, cuda), ce).cpu().numpy()
    assert np.array_equal(got, want) and np.isfinite(want).all() and want.std() > 0.01
