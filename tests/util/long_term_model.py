"""Long-term priors (Ruder, Dosovitskiy, Brox 2016, section 4.2) restated in numpy: the per-pixel weights, the merged network input of
csrc/kernels_longterm.hip in its own operation order (fp32) and in fp64, the model of a stream's frame (check, erosion, merge per
distance), and the synthetic "occluder" scene whose ground-truth flows make the feature's effect countable.

Builds on the oracle's warp, consistency check, erosion and pre-processing and on tests/util/frame_input_model.py's inputs."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_input_model as M  # noqa: E402

MEAN = M.MEAN
F = np.float32


def weights(c, dtype=np.float32):
    """c [K][...] certainties in ascending distance -> (w [K][...], C): w_k = max(c_k - sum_{j<k} c_j, 0), C = sum_k w_k,
    every operation rounded to dtype in the kernel's order (used = used + c_k; C = C + w_k)"""
    c = np.asarray(c, dtype)
    used = np.zeros(c.shape[1:], dtype); C = np.zeros(c.shape[1:], dtype)
    w = np.empty_like(c)
    for k in range(c.shape[0]):
        w[k] = np.maximum(c[k] - used, dtype(0))
        used = used + c[k]
        C = C + w[k]
    return w, C


def merge_input(O, frame_u8, states, flows, certs, border="stn", fill_random=False, seed=0, index=0, dtype=np.float32):
    """the [7][H][W] network input from K priors (states [3][Hs][Ws], flows [H][W][2] (u, v), certs [H][W] eroded) and the merged
    certainty C.  dtype float32: the kernel's arithmetic operation by operation (a prior whose weight is 0 at a pixel contributes
    nothing there, whatever its warp gives); float64: the same formula on the fp32 warps, for the tolerance of the weights"""
    from vr_oracle import fill_uniform
    h, w_ = frame_u8.shape[:2]
    mode = "stn_f32" if border == "stn" else "cpu"
    frame01 = frame_u8.astype(np.float32) / np.float32(255)
    x = np.empty((7, h, w_), dtype)
    for c in range(3):
        x[c] = frame01[..., 2 - c] * np.float32(255.0) - MEAN[c]              # content: fp32 in both versions (bit-equal on the GPU)
    w, C = weights(np.stack(certs), dtype)
    acc = np.zeros((3, h, w_), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(states)):
            warped = O.warp(states[k], O.flo_to_lua(flows[k]), mode).astype(dtype)   # [3][H][W] RGB on the flow's grid
            for c in range(3):
                term = (warped[2 - c] * dtype(255.0) - dtype(MEAN[c])) * w[k]
                acc[c] = acc[c] + np.where(w[k] == 0, dtype(0), term)
    cinv = (C + dtype(-1)) * dtype(-1)
    for c in range(3):
        fill = dtype(0)
        if fill_random:
            u = fill_uniform(seed, index, h, w_)[2 - c].astype(dtype)
            fill = (u * dtype(255.0) - dtype(MEAN[c])) * cinv
        x[3 + c] = fill + acc[c]
    x[6] = C
    return x, C


def eroded_certainty(O, bw, fw, r=7, frame_u8=None):
    """mask byte of the forward-backward check (3-argument, or 4-argument with the frame) and its eroded certainty, default options"""
    m = O.consistency(bw, fw, frame_u8) if frame_u8 is not None else O.consistency(bw, fw)
    return m, O.min_filter(m.astype(np.float32) / np.float32(255), r)


def stream_input(O, frame_u8, states, bws, fws, r=7, border="stn", fill_random=False, seed=0, index=0, dtype=np.float32):
    """what fav_stream_next_frame_flows_lt assembles: per distance the check and the erosion, then the merge -> (x [7][H][W], masks)"""
    masks, certs = zip(*[eroded_certainty(O, b, f, r) for b, f in zip(bws, fws)])
    x, _ = merge_input(O, frame_u8, states, bws, list(certs), border, fill_random, seed, index, dtype)
    return x, list(masks)


# ----------------------------------------------------------------------------------------------------------------- occluder scene
SCENE_H, SCENE_W, BAR_W, BAR_STEP, BAR_X0 = 48, 96, 10, 10, 8


def bar_x(i):
    """left edge of the bar in frame i (it spans the frame's height)"""
    return BAR_X0 + BAR_STEP * i


def scene_frame(i, h=SCENE_H, w=SCENE_W):
    """frame i, u8 [H][W][3]: a textured static background and an opaque bar with its own texture, BAR_W wide, BAR_STEP px per frame"""
    from fav_amd import synth
    bg = (synth.smooth_frame(h, w, 41).astype(np.int32) * 3 // 4 + synth.random_frame(h, w, 42).astype(np.int32) // 4).astype(np.uint8)
    bar = (255 - synth.smooth_frame(h, BAR_W, 43).astype(np.int32) // 2).astype(np.uint8)
    f = bg.copy()
    f[:, bar_x(i):bar_x(i) + BAR_W] = bar
    return f


def scene_flows(i, d, h=SCENE_H, w=SCENE_W):
    """ground truth between frames i and i - d: (backward [H][W][2] with A = frame i, forward with A = frame i - d), (u, v)"""
    bw = np.zeros((h, w, 2), np.float32); fw = np.zeros((h, w, 2), np.float32)
    bw[:, bar_x(i):bar_x(i) + BAR_W, 0] = -BAR_STEP * d
    fw[:, bar_x(i - d):bar_x(i - d) + BAR_W, 0] = BAR_STEP * d
    return bw, fw


def uncovered(i, h=SCENE_H, w=SCENE_W):
    """the background pixels the bar covered in frame i - 1 and no longer covers in frame i"""
    m = np.zeros((h, w), bool)
    m[:, bar_x(i - 1):bar_x(i - 1) + BAR_W] = True
    m[:, bar_x(i):bar_x(i) + BAR_W] = False
    return m


def scene_certainties(O, i, distances, r=7):
    """eroded certainties of frame i towards i - d for the distances the scene can serve (d <= i)"""
    return [eroded_certainty(O, *scene_flows(i, d), r)[1] for d in distances if d <= i]
