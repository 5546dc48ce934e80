"""Host side of -scene_cut (no GPU needed): the numpy model of the block-histogram distance (tests/util/scene_model.py) against the
properties its definition promises, the six-frame clip that the GPU tests stylise -- whose scores are what justifies their threshold of
0.5 -- and the combinations of -scene_cut / -scene_cut_log that fav_stylize refuses before it opens a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import scene_model as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")


def _const(w, h, rgb):
    a = np.empty((h, w, 3), np.uint8)
    a[...] = rgb
    return a


# ------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("size", [(4, 4), (13, 7), (67, 35), (256, 64)], ids=lambda s: "%dx%d" % s)
def test_identical_frames_give_zero(size):
    w, h = size
    a = np.random.default_rng(w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert S.scene_change(a, a) == (0, [0] * 16) and S.scene_change(a, a.copy()) == (0, [0] * 16)


@pytest.mark.parametrize("size", [(4, 4), (13, 7), (67, 35)], ids=lambda s: "%dx%d" % s)
def test_constant_frames_in_different_bins_give_twice_the_pixels(size):
    w, h = size
    a, b = _const(w, h, (0, 0, 0)), _const(w, h, (255, 255, 255))
    assert int(S.luma(a)[0, 0]) == 0 and int(S.luma(b)[0, 0]) == 255                # the luma weights sum to 256: white is 255
    total, cells = S.scene_change(a, b)
    assert total == 2 * w * h and S.score(a, b) == 1.0
    # ... and in the SAME bin (lumas 8 and 15 are both bin 1) nothing
    assert int(S.luma(_const(w, h, (8, 8, 8)))[0, 0]) == 8 and int(S.luma(_const(w, h, (15, 15, 15)))[0, 0]) == 15
    assert S.scene_change(_const(w, h, (8, 8, 8)), _const(w, h, (15, 15, 15)))[0] == 0


def test_luma_is_the_stated_integer_form():
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    want = [(77 * int(r) + 150 * int(g) + 29 * int(b) + 128) >> 8 for r, g, b in p]
    assert S.luma(p.reshape(50, 1, 3)).reshape(-1).tolist() == want and max(want) <= 255


@pytest.mark.parametrize("size", [(4, 4), (13, 7), (67, 35), (256, 64)], ids=lambda s: "%dx%d" % s)
def test_cells_sum_to_the_total(size):
    w, h = size
    rng = np.random.default_rng(h)
    a, b = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2))
    total, cells = S.scene_change(a, b)
    assert len(cells) == 16 and sum(cells) == total and 0 < total <= 2 * w * h
    assert S.scene_change(b, a) == (total, cells)                                   # |.| is symmetric


def test_cell_boundaries_of_13x7_are_the_floor_division_ones():
    assert S.cell_bounds(13) == [0, 3, 6, 9, 13] and S.cell_bounds(7) == [0, 1, 3, 5, 7]
    w, h = 13, 7
    a = _const(w, h, (0, 0, 0))
    # one white pixel moves exactly its own cell: 2 (it left bin 0 and entered bin 31)
    for y in range(h):
        for x in range(w):
            b = a.copy(); b[y, x] = 255
            cx = sum(x >= v for v in (3, 6, 9)); cy = sum(y >= v for v in (1, 3, 5))
            total, cells = S.scene_change(a, b)
            assert total == 2 and cells[cy * 4 + cx] == 2, (x, y)
    # the sizes of the cells, from a white frame against a black one
    _, cells = S.scene_change(a, _const(w, h, (255, 255, 255)))
    assert cells == [2 * cw * ch for ch in (1, 2, 2, 2) for cw in (3, 3, 3, 4)]


def test_cells_separate_scenes_whose_global_histograms_coincide():
    a = _const(16, 16, (0, 0, 0)); a[:, 8:] = 255
    b = a[:, ::-1].copy()                                                           # mirrored: the same global histogram
    assert np.array_equal(np.bincount(S.luma(a).reshape(-1), minlength=256), np.bincount(S.luma(b).reshape(-1), minlength=256))
    assert S.score(a, b) == 1.0


def test_motion_inside_a_cell_is_not_seen():
    a = _const(32, 32, (0, 0, 0)); a[2:5, 2:5] = 255
    b = _const(32, 32, (0, 0, 0)); b[3:6, 4:7] = 255                                # the square moved, and stayed in cell (0, 0)
    assert S.scene_change(a, b)[0] == 0


# ------------------------------------------------------------------------------------------------ 2. the test clip
def test_clip_scores_justify_the_threshold_of_the_gpu_tests():
    """T = 0.5 in tests/test_gpu_scene_cut.py: every pair inside a scene stays below 0.25, the pair across the cut is above 0.75"""
    clip = S.cut_clip()
    assert len(clip) == 6 and all(f.shape == (S.CLIP_H, S.CLIP_W, 3) and f.dtype == np.uint8 for f in clip)
    scores = [S.score(clip[k - 1], clip[k]) for k in range(1, 6)]
    print("scores of the clip's neighbouring pairs:", ["%.4f" % s for s in scores])
    for k in (0, 1, 3, 4):
        assert scores[k] < 0.25, scores
    assert scores[2] > 0.75, scores
    # scene A is mid-to-bright, scene B dark; inside a scene the picture translates by one pixel
    assert min(int(S.luma(f).min()) for f in clip[:3]) >= 120 and max(int(S.luma(f).max()) for f in clip[3:]) <= 110
    for k in (0, 1, 3, 4):
        assert np.array_equal(clip[k][:, 1:], clip[k + 1][:, :-1]) and not np.array_equal(clip[k], clip[k + 1])
    # ... and in the reverse order (-backward) the cut sits between frames 4 and 3
    back = clip[::-1]
    assert [S.score(back[k - 1], back[k]) > 0.5 for k in range(1, 6)] == [False, False, True, False, False]


# ------------------------------------------------------------------------------------------------ 3. fav_stylize: refused before a device is opened
@pytest.mark.parametrize("args,msg", [
    (["-scene_cut", "0.5", "-flow_pattern", "bw_[%d]_{%d}.flo", "-occlusions_pattern", "r_[%d]_{%d}.pgm"], "-scene_cut 0.5 needs -estimate_flow 1"),
    (["-scene_cut", "0.5", "-estimate_flow", "1", "-create_inconsistent"], "cannot be combined with -create_inconsistent"),
    (["-scene_cut", "1.5", "-estimate_flow", "1"], "-scene_cut must be a number in [0, 1]"),
    (["-scene_cut", "-0.1", "-estimate_flow", "1"], "-scene_cut must be a number in [0, 1]"),
    (["-scene_cut", "half", "-estimate_flow", "1"], "-scene_cut must be a number in [0, 1]"),
    (["-scene_cut", "nan", "-estimate_flow", "1"], "-scene_cut must be a number in [0, 1]"),
    (["-scene_cut_log", "cuts.txt", "-estimate_flow", "1"], "-scene_cut_log needs -scene_cut"),
    (["-scene_cut_log", "cuts.txt", "-scene_cut", "0", "-estimate_flow", "1"], "-scene_cut_log needs -scene_cut"),
])
def test_fav_stylize_refuses_before_the_device(tmp_path, args, msg):
    if not os.path.exists(STYLIZE):
        pytest.skip("fav_stylize is not built")
    r = subprocess.run([STYLIZE, "-input_pattern", "f_%05d.ppm"] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL, cwd=tmp_path)
    assert r.returncode != 0 and msg in r.stderr, r.stderr
    assert "HIP" not in r.stderr and r.stdout == ""
    assert os.listdir(tmp_path) == [], "a refused run left files behind"


def test_abi_and_binding_carry_the_operator(favlib):
    hdr = open(os.path.join(ROOT, "include", "fav.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("fav_scene_change_workspace_bytes", "fav_scene_change_rgb8"):
        assert name in favlib.EXPORTS and hasattr(favlib.lib(), name) and name + "(" in hdr and name in integration, name
    assert favlib.scene_change_workspace_bytes() == 16 * 32 * 4 and callable(favlib.scene_change)
