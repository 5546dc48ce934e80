"""numpy restatement of csrc/kernels_scene.hip ("Scene changes"): the block-histogram distance of two RGB8 frames behind
fav_stylize -scene_cut.  Integer arithmetic throughout, so the kernel is held to this model for equality:
    luma  Y = (77 R + 150 G + 29 B + 128) >> 8,  bin = Y >> 3  (32 bins)
    grid  4 x 4 cells, cell (cx, cy) = x in [cx W/4, (cx+1) W/4), y in [cy H/4, (cy+1) H/4), floor division (W, H >= 4)
    cell[cy*4+cx] = sum over bins |hist_prev - hist_cur|,  total = sum over cells,  score = total / (2 W H)
Also the six-frame clip with one cut that the CLI tests stylise."""
import numpy as np

BINS, GRID = 32, 4


def luma(rgb_hwc):
    """[H][W][3] u8 -> Y [H][W], 0..255"""
    p = np.asarray(rgb_hwc).astype(np.int64)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def cell_bounds(n):
    """the five boundaries of the four cells along a side of n samples: cell c covers [b[c], b[c+1])"""
    return [c * n // GRID for c in range(GRID + 1)]


def histograms(rgb_hwc):
    """[16][32] int64: the luma histogram of every cell, cell index cy*4+cx"""
    y = luma(rgb_hwc) >> 3
    h, w = y.shape
    assert w >= GRID and h >= GRID, "4 x 4 cells need a frame of at least 4 x 4"
    bx, by = cell_bounds(w), cell_bounds(h)
    out = np.zeros((GRID * GRID, BINS), np.int64)
    for cy in range(GRID):
        for cx in range(GRID):
            out[cy * GRID + cx] = np.bincount(y[by[cy]:by[cy + 1], bx[cx]:bx[cx + 1]].reshape(-1), minlength=BINS)
    return out


def scene_change(prev, cur):
    """-> (total, cells): what fav_scene_change_rgb8 leaves in fav_scene_change"""
    assert np.shape(prev) == np.shape(cur)
    cells = np.abs(histograms(prev) - histograms(cur)).sum(axis=1)
    return int(cells.sum()), [int(v) for v in cells]


def score(prev, cur):
    h, w = np.shape(prev)[:2]
    return scene_change(prev, cur)[0] / (2.0 * w * h)


# ---------------------------------------------------------------------------------------------- the test clip
CLIP_W, CLIP_H = 64, 48


def _texture(h, w, seed, lo, hi):
    """a smooth texture (the blurred noise of fav_amd.synth.smooth_frame) with every channel in lo..hi, 8 columns wider than the
    frame: the clip's frames are windows into it"""
    from fav_amd import synth
    a = synth.smooth_frame(h, w + 8, seed).astype(np.float64) / 255.0
    return (lo + a * (hi - lo)).astype(np.uint8)


def cut_clip():
    """six 64 x 48 frames: 1-3 are scene A (mid-to-bright luma, 128..250), 4-6 scene B (another texture, dark luma, 5..100); inside a
    scene the picture translates by 1 px per frame"""
    a, b = _texture(CLIP_H, CLIP_W, 11, 128, 250), _texture(CLIP_H, CLIP_W, 23, 5, 100)
    return [np.ascontiguousarray(t[:, k:k + CLIP_W]) for t in (a, b) for k in range(3)]


def write_ppm(path, rgb_hwc):
    h, w = rgb_hwc.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(rgb_hwc, np.uint8).tobytes())
