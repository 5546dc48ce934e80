"""Long-term priors without a GPU: the weights' algebra, the occluder scene the GPU tests run (does it have the pixels the feature is
about?), and fav_stylize's refusals of -long_term, which precede every use of a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import long_term_model as LT  # noqa: E402

BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_weights(K):
    rng = np.random.default_rng(100 + K)
    c = rng.random((K, 4096)).astype(np.float32)
    c[:, :64] = rng.integers(0, 2, (K, 64))                    # the checker's own certainties: 0 and 1
    c[0, 64:128] = 1.0                                          # certain at distance 1
    if K > 1:
        c[0, 128:192] = 0.0; c[1, 128:192] = 1.0                # occluded at distance 1, visible at the next
    w, C = LT.weights(c)
    w64, C64 = LT.weights(c, np.float64)
    assert w.dtype == np.float32 and (w >= 0).all()
    assert np.array_equal(w[0], c[0])
    # sum w <= max c <= 1: exact in fp64; fp32 rounds each of the at most 2 (K - 1) additions that matter by half an ulp of a value <= 4
    assert (w64.sum(0) <= c.astype(np.float64).max(0) + 1e-15).all() and (c.max(0) <= 1).all()
    assert (C <= c.max(0) + 4 * K * np.finfo(np.float32).eps).all() and (C <= 1 + 4 * K * np.finfo(np.float32).eps).all()
    assert not w[1:, 64:128].any()                               # c_0 = 1: nothing further back is used
    if K > 1:
        assert (w[1, 128:192] == 1).all() and not w[2:, 128:192].any()
    # a few ulps of the largest intermediate (used <= K): each of the <= 3 K operations rounds once
    tol = 3 * K * K * np.finfo(np.float32).eps
    assert np.abs(w - w64).max() <= tol and np.abs(C - C64).max() <= tol


def test_occluder_scene(oracle):
    """with ground-truth flows the pixels uncovered at frame i are occluded at distance 1 and visible at distance 2 (apart from the
    erosion ring); J = {1, 2} raises the merged certainty exactly there, and lowers it nowhere"""
    assert LT.bar_x(6) + LT.BAR_W <= LT.SCENE_W
    for i in range(2, 7):
        c1, c2 = LT.scene_certainties(oracle, i, (1, 2))
        assert set(np.unique(c1)) <= {0.0, 1.0} and set(np.unique(c2)) <= {0.0, 1.0}
        _, C1 = LT.weights(np.stack([c1]))
        _, C12 = LT.weights(np.stack([c1, c2]))
        gained = C12 > C1
        assert not (C12 < C1).any()
        assert np.array_equal(gained, (c1 == 0) & (c2 == 1))
        unc = LT.uncovered(i)
        assert not c1[unc].any(), "an uncovered pixel is certain at distance 1"
        # the scene really has such pixels with the default window 7: whole columns of them through the 16 rows of a tile, in the first two
        # tile rows (the checker distrusts the frame's last row and column at every distance -- a bilinear tap lies outside -- and the
        # erosion widens that to four rows, inside the third tile row)
        for ty in (0, 1):
            cols = np.flatnonzero((gained & unc)[16 * ty:16 * ty + 16].all(axis=0))
            assert len(cols) >= 3, f"frame {i}, tile row {ty}: {len(cols)} full tile columns of uncovered pixels gain certainty"
        assert (gained & unc)[:LT.SCENE_H - 4].all(axis=0).sum() >= 3 and not c2[LT.SCENE_H - 4:].any()
        assert (gained <= ~(c1 > 0)).all()
        # fp64 model of the merge on these certainties: the share of pixels without any prior falls
        assert (C12 == 0).mean() < (C1 == 0).mean()


def _cli(tmp_path, *extra):
    from fav_amd import synth
    import oracle as O
    for i in (1, 2):
        O.write_pnm(str(tmp_path / f"frame_{i:05d}.ppm"), synth.smooth_frame(48, 64, i))
    os.makedirs(tmp_path / "out", exist_ok=True)
    cmd = [os.path.join(BIN, "fav_stylize"), "-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-output_prefix", str(tmp_path / "out" / "out"),
           "-model_vid", os.path.join(ROOT, "tests", "golden", "tiny_model.t7"), "-model_img", "self", "-gpu", "0"] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


REFUSED = [
    (["-long_term", "2", "-flow_pattern", "f_[%d]_{%d}.flo", "-occlusions_pattern", "o_[%d]_{%d}.pgm"], "needs -estimate_flow 1"),
    (["-long_term", "2,4", "-estimate_flow", "1", "-create_inconsistent"], "cannot be combined with -create_inconsistent"),
    (["-long_term", "1", "-estimate_flow", "1"], "-long_term must list"),
    (["-long_term", "4,2", "-estimate_flow", "1"], "-long_term must list"),
    (["-long_term", "2,2", "-estimate_flow", "1"], "-long_term must list"),
    (["-long_term", "17", "-estimate_flow", "1"], "-long_term must list"),
    (["-long_term", "2,3,4,5", "-estimate_flow", "1"], "-long_term must list"),
    (["-long_term", "2,", "-estimate_flow", "1"], "-long_term must list"),
    (["-long_term", "2;4", "-estimate_flow", "1"], "-long_term must list"),
    (["-long_term", "x", "-estimate_flow", "1"], "-long_term must list"),
]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=[" ".join(e[:2]) + ("+" + e[-1].lstrip("-") if len(e) % 2 else "") + f"#{k}" for k, (e, _) in enumerate(REFUSED)])
def test_fav_stylize_refuses(oracle, favlib, tmp_path, extra, msg):
    r = _cli(tmp_path, *extra)
    assert r.returncode == 1 and msg in r.stderr, (r.returncode, r.stderr)
    assert os.listdir(tmp_path / "out") == []
