"""The two CPU statements of the 360-degree post-processing held to each other (no GPU): tests/util/vr_post_model.py (index formulas,
sorted strided view) against oracle/vr_oracle.py (transposes, reversals, unfolded copy) -- median_filter, the three rotations, and
VRStylizer._finish's filtered faces, equirectangular input strip and cube-map strip -- on inputs the GPU tests had never seen: ties in
every window, +-inf, values outside [0, 1], asymmetric overlaps.  tests/test_gpu_vr_post.py then holds the GPU to the model bit for bit.

The reference cannot be run here (no Lua/Torch7 on this project's machines).  What decides the median is
fast_artistic_video/utils.lua:157, `u:view(3, HH, WW, r * r):float():median()`: torch's median over the last dimension of r*r elements,
which for an odd count is the middle element of the sorted window and in general the LOWER median, index (r*r - 1) // 2 [recalled from
Torch7's documentation of torch.median; also oracle/vr_oracle.py's header].  test_median_on_hand_computed_windows records cases worked
out by hand from that line.  What such a median returns for a window that holds a NaN is not defined by utils.lua (it is whatever
TH's selection does with unordered comparisons): the GPU tests leave such windows out, and DESIGN.md says so."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import vr_post_model as M  # noqa: E402

F = np.float32
N = 260                                    # the GPU tests' main face size


@pytest.fixture(scope="module")
def V(oracle):
    import vr_oracle
    return vr_oracle


def _finish(V, faces, hp, wp, **kw):
    chk = V.VRStylizer(None, hp, wp, **kw)
    chk.last = faces
    chk._finish()
    return chk


def test_median_on_hand_computed_windows():
    """utils.lua:157 on windows small enough to sort by hand"""
    w = np.array([[9, 1, 8], [2, 7, 3], [6, 4, 5]], F)                       # sorted 1..9 -> the 5th smallest
    assert M.median(np.stack([w] * 3), 3).ravel().tolist() == [5, 5, 5]
    t = np.array([[1, 0, 1], [0, 1, 0], [1, 0, 1]], F)                       # 0 0 0 0 | 1 1 1 1 1 -> index 4 is the first 1
    assert M.median(np.stack([t] * 3), 3).ravel().tolist() == [1, 1, 1]
    t = 1 - t                                                                # 0 0 0 0 0 | 1 1 1 1 -> index 4 is the last 0
    assert M.median(np.stack([t] * 3), 3).ravel().tolist() == [0, 0, 0]
    i = np.array([[-np.inf, np.inf, 3], [np.inf, -np.inf, 2], [np.inf, 1, -np.inf]], F)   # -inf x3, 1, 2, 3, inf x3 -> 2
    assert M.median(np.stack([i] * 3), 3).ravel().tolist() == [2, 2, 2]
    v = np.arange(25, dtype=F)[::-1].reshape(5, 5) * F(0.5)                  # 0 .. 12 in halves -> index 12 = 6
    assert M.median(np.stack([v] * 3), 5).ravel().tolist() == [6, 6, 6]
    two = np.zeros((3, 3, 4), F); two[:, :, 3] = 7                           # [3][3][4]: two windows along x: 0 x9; 0 x6 + 7 x3
    assert M.median(two, 3).shape == (3, 1, 2) and M.median(two, 3).ravel().tolist() == [0, 0] * 3


@pytest.mark.parametrize("variant", ["coded", "ties", "inf", "range"])
@pytest.mark.parametrize("r", [3, 5])
def test_median_model_equals_oracle(V, variant, r):
    for f in M.faces(68, variant)[:3]:
        a, b = M.median(f, r), V.median_filter(f, r)
        assert a.shape == (3, 68 - r + 1, 68 - r + 1) and a.dtype == F
        assert np.array_equal(a, b)
    odd = M.faces(68, variant)[4][:, :37, :51]                               # not square
    assert np.array_equal(M.median(odd, r), V.median_filter(odd, r))


def test_median_of_a_coded_window_is_its_centre():
    for r in (3, 5):
        f = M.coded_face(40, 3)
        assert np.array_equal(M.median(f, r), f[:, r // 2:40 - r // 2, r // 2:40 - r // 2])


def test_every_window_of_the_ties_variant_has_ties():
    for f in M.faces(68, "ties"):
        win = np.lib.stride_tricks.sliding_window_view(f, (3, 3), axis=(1, 2)).reshape(3, 66, 66, 9)
        assert (np.sort(win, -1)[..., 1:] == np.sort(win, -1)[..., :-1]).any(-1).all()
        assert len(np.unique(f)) == 8


def test_rotations_model_equals_oracle(V):
    t = np.arange(3 * 5 * 7, dtype=F).reshape(3, 5, 7)
    assert np.array_equal(M.rotate(t, 1), V.rotate90(t)) and M.rotate(t, 1).shape == (3, 7, 5)
    assert np.array_equal(M.rotate(t, 2), V.rotate_minus90(t))
    assert np.array_equal(M.rotate(t, 3), V.rotate180(t))
    assert np.array_equal(M.rotate(t, 0), t)
    assert np.array_equal(M.rotate(M.rotate(t, 1), 2), t) and np.array_equal(M.rotate(M.rotate(t, 1), 1), M.rotate(t, 3))
    assert M.rotate(t, 1)[0, 0, 0] == t[0, 0, 6] and M.rotate(t, 2)[0, 0, 0] == t[0, 4, 0]      # the formulas, at one corner each


def test_decode_inverts_the_code():
    for k in (0, 5):
        f = M.coded_face(N, k)
        y, x = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        for c in range(3):
            fk, fy, fx = M.decode(f[c], c)
            assert (fk == k).all() and np.array_equal(fy, y) and np.array_equal(fx, x)
        assert (M.decode(f[1], 0)[0] != k).any() and (M.decode(f[0] + F(2.0 ** -24), 0)[0] == -1).all()
    assert f.min() >= 0 and f.max() < 1


@pytest.mark.parametrize("med", [0, 3, 5])
@pytest.mark.parametrize("variant", ["coded", "ties", "inf", "range"])
def test_finish_model_equals_oracle_square(V, oracle, med, variant):
    """24/24 on 68x68 faces: filtered faces, cube-map strip and the equirectangular image of the model's input strip"""
    n = 68
    kw = dict(overlap_w=24, overlap_h=24, median=med, out_equi_w=96, out_equi_h=48)
    chk = _finish(V, M.faces(n, variant), n, n, **kw)
    filt = [M.median(b, med) for b in chk.blended]
    for k in range(6):
        assert np.array_equal(filt[k], chk.filtered[k], equal_nan=True)
    assert np.array_equal(M.cube_strip(filt, n, n, 24, 24, med), chk.cubemap, equal_nan=True)
    assert np.array_equal(V.warp(M.equi_strip(filt), chk.equi_map), chk.equi, equal_nan=True)
    if variant != "inf":
        assert np.array_equal(M.quantize(chk.cubemap), oracle.to_u8_hwc(chk.cubemap))
        assert np.array_equal(M.quantize(chk.equi), oracle.to_u8_hwc(chk.equi))


@pytest.mark.parametrize("med", [0, 3, 5])
@pytest.mark.parametrize("ow,oh", [(12, 40), (40, 12)])
def test_finish_model_equals_oracle_asymmetric(V, oracle, med, ow, oh):
    """asymmetric overlaps.  On a square face the crops are not square and both statements refuse the cube map; the face sizes at
    which the crops ARE square (hp - overlap_h == wp - overlap_w) tell a crop that mixes the two overlaps from the right one."""
    n = 64
    kw = dict(overlap_w=ow, overlap_h=oh, median=med, out_equi_w=96, out_equi_h=48)
    with pytest.raises(ValueError):
        _finish(V, M.faces(n, "ties"), n, n, **kw)
    filt = [M.median(f, med) for f in M.faces(n, "ties")]
    with pytest.raises(ValueError, match="square"):
        M.cube_strip(filt, n, n, ow, oh, med)
    hp, wp = n + oh, n + ow
    rng = np.random.default_rng(5)
    chk = _finish(V, [rng.integers(0, 8, (3, hp, wp)).astype(F) / F(8) for _ in range(6)], hp, wp, **kw)
    filt = [M.median(b, med) for b in chk.blended]
    for k in range(6):
        assert np.array_equal(filt[k], chk.filtered[k])
    ovh, ovw, ch, cw = M.cube_crop(hp, wp, ow, oh, med)
    assert (ovh, ovw, ch, cw) == (oh // 2 - med // 2, ow // 2 - med // 2, n + 2 * (med // 2), n + 2 * (med // 2))
    assert np.array_equal(M.cube_strip(filt, hp, wp, ow, oh, med), chk.cubemap) and chk.cubemap.shape == (3, ch, 6 * cw)
    assert np.array_equal(V.warp(M.equi_strip(filt), chk.equi_map), chk.equi)


def test_quantize_model_equals_oracle_on_specials(oracle):
    img = np.zeros((3, 2, len(M.SPECIALS)), F)
    img[:, 0] = np.array(M.SPECIALS, F); img[:, 1] = np.array([np.inf, -np.inf] * (len(M.SPECIALS) // 2), F)
    q = M.quantize(img)
    assert np.array_equal(q, oracle.to_u8_hwc(img))
    want = {-0.0: 0, 1.0: 255, 254.999 / 255: 254, 255.001 / 255: 255, 1 / 255: 1, 0.999 / 255: 0, 1 + 1e-7: 255, 1e-40: 0, 2.0: 255, -5.0: 0, 0.5: 127}
    for v, b in want.items():
        assert q[0, M.SPECIALS.index(v), 0] == b, (v, b)
    assert q[1, 0, 0] == 255 and q[1, 1, 0] == 0
    f = M.faces(68, "range")[2]
    assert np.array_equal(M.quantize(f), oracle.to_u8_hwc(f)) and f.min() < -0.4 and f.max() > 1.4
    assert M.quantize(np.full((3, 1, 1), np.nan, F)).ravel().tolist() == [0, 0, 0]


@pytest.mark.parametrize("med", [0, 3, 5])
def test_cube_sources_is_the_strip_of_coded_faces(med):
    """the model-free source table against the model's strip of (unblended) coded faces: every pixel, not only the interior"""
    n = 68
    filt = [M.median(f, med) for f in M.faces(n, "coded")]
    strip = M.cube_strip(filt, n, n, 24, 24, med)
    face, y, x, interior = M.cube_sources(n, 24, 24, med)
    for c in range(3):
        fk, fy, fx = M.decode(strip[c], c)
        assert np.array_equal(fk, face) and np.array_equal(fy, y) and np.array_equal(fx, x)
    assert 0.3 < interior.mean() < 1 and not interior[:, 0].any()


@pytest.mark.parametrize("variant", ["nan", "inf"])
def test_non_finite_values_stay_in_their_own_face(V, variant):
    """what the NaN cap of the GPU test rests on, on the oracle alone: the blend's warps sample no pixel of the middle half of a
    neighbour, so the blended faces are non-finite exactly where the raw faces are -- 20 NaNs per plane, at most 20 r^2 windows"""
    faces = M.faces(N, variant)
    chk = _finish(V, faces, N, N, overlap_w=24, overlap_h=24, median=0)
    for k in range(6):
        assert np.array_equal(np.isfinite(chk.blended[k]), np.isfinite(faces[k]))
        assert np.array_equal(chk.blended[k][~np.isfinite(faces[k])], faces[k][~np.isfinite(faces[k])], equal_nan=True)
        if variant == "nan":
            pos = M.nan_positions(N, k)
            assert len(set(pos)) == M.NAN_PER_FACE
            assert min(max(abs(a[0] - b[0]), abs(a[1] - b[1])) for a in pos for b in pos if a != b) > 5
            for r in (3, 5):
                per_plane = M.nan_windows(chk.blended[k], r).sum(axis=(1, 2))
                assert (per_plane == M.NAN_PER_FACE * r * r).all() and per_plane.max() < 0.01 * (N - r + 1) ** 2
        else:
            assert 0.002 < (~np.isfinite(faces[k])).mean() < 0.02 and (faces[k] == np.inf).any() and (faces[k] == -np.inf).any()
