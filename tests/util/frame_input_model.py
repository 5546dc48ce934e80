"""Inputs, option lattice, GPU driver and CPU model of tests/test_gpu_frame_input.py: the eight floats per pixel a frame's network input
holds, on every route of the stream (mask file, fused check, look-ahead, the diagnostic two-launch form).

The driver (run_route) runs in the test's own process and -- for the two-launch route, whose switch the library reads once per
process -- as a child:  python frame_input_model.py <route> <net.t7> <in.npz> <out.npz>."""
import itertools
import os
import sys

import numpy as np

MEAN = np.array([103.939, 116.779, 123.68], np.float32)        # BGR (preprocess.lua:57-62)
TILE_Y, TILE_X = 16, 64                                        # the erosion kernels' tile (MF_TY x MF_TX)
R_ALL = (1, 2, 7, 8, 15)                                    # erosion windows: odd, even, the default 7 and the largest
FILLS = ((0, 1), (1, 5), (1, 6))                               # (fill_random, seed): vgg-mean, uniform-random with two seeds
ROUTES = ("cert", "flow3", "flow4", "lookahead", "lookahead-host", "two-launch")
MASK_OF = {"cert": "grey", "flow3": "m3", "flow4": "m4", "lookahead": "m4", "lookahead-host": "m4", "two-launch": "m3"}


def option_sets(rs):
    """(kind, border, invert, fix, fill_random, seed, r): flow (a) under both borders, flow (b) under the STN border only"""
    out = []
    for kind, border in (("a", "stn"), ("a", "cpu"), ("b", "stn")):
        for inv, fix, (fill, seed), r in itertools.product((0, 1), (0, 1), FILLS, rs):
            out.append((kind, border, inv, fix, fill, seed, r))
    return out


def quantised_flow(h, w, seed):
    """flow (a): smooth random motion on the grid of multiples of 1/8, |flow| < 32 -- every bilinear weight and every sum of weights is
    exact in fp32 -- plus a band that leaves the image by exactly half a pixel (all-ones warp = 0.5 under the STN border: sign 0) on the
    first row and the first column, and a band that leaves it entirely on the last row.  Frames smaller than two tiles move by less
    than a pixel, so that -fix_occlusions and the CPU border blank the outermost ring only and the widest window still sees certainty."""
    from fav_amd import synth
    f = synth.backward_flow(h, w, seed).astype(np.float64)
    if min(h, w) < 2 * TILE_Y:
        f = f / np.abs(f).max() * 0.875
    f = np.clip(np.round(f * 8) / 8, -31.875, 31.875).astype(np.float32)
    f[0, :w // 2] = (0.0, -0.5)                                # (u, v) = (dx, dy): half a pixel above the image
    f[h // 3:2 * h // 3, 0] = (-0.5, 0.0)                      # half a pixel left of it
    f[h - 1, :w // 2] = (0.0, 8.0)                             # eight rows below it
    assert np.array_equal(f * 8, np.round(f * 8)) and np.abs(f).max() < 32
    return f


def wild_flow(h, w, seed):
    """flow (b): unrestricted random motion; the first rows carry the non-finite and huge entries of
    test_fused_prior_bit_exact_vs_reference_kernel (NaN, +-inf, 2^31, -3e9, 1e20)"""
    f = (np.random.default_rng(seed).standard_normal((h, w, 2)) * 4).astype(np.float32)
    f[0, :6] = [[0.0, -1.5], [-0.5, -1.5], [0.25, -0.5], [-2.0, 0.0], [np.inf, 0.0], [np.nan, 1.0]]
    f[-1, -3:] = 0.75
    f[5, :4] = [[2.0 ** 31, 0.0], [-3e9, 0.5], [0.0, 1e20], [0.0, -np.inf]]
    return f


def grey_mask(h, w, seed):
    """certainty bytes of the mask-file route: uniform over 0..255, with zeros on the tile seams, in the four corners and on each edge
    (within r/2 of it for every window)"""
    m = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    for y in range(TILE_Y, h, TILE_Y):
        m[y - 1:y + 1, 0] = 0
        m[y - 1:y + 1, w - 1] = 0
    for x in range(TILE_X, w, TILE_X):
        m[0:2, x - 1:x + 1] = 0
        m[h - 1, x - 1:x + 1] = 0
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)):
        m[y, x] = 0
    return m


def make_inputs(O, h, w, ho, wo, seed):
    """everything one size needs, as a dict of arrays (what the two-launch child reads from its .npz)"""
    from fav_amd import synth
    rng = np.random.default_rng(seed)
    frame = synth.random_frame(h, w, seed + 1)
    state = (rng.standard_normal((3, ho, wo)) * 0.4 + 0.5).astype(np.float32)          # unclamped: some values below 0 and above 1
    bw_a, bw_b = quantised_flow(h, w, seed + 2), wild_flow(h, w, seed + 3)
    fw = synth.forward_flow_from_backward(bw_a, seed + 4)
    d = dict(frame=frame, state=state, bw_a=bw_a, bw_b=bw_b, fw=fw, grey=grey_mask(h, w, seed + 5))
    for k in "ab":
        d["m3_" + k] = O.consistency(d["bw_" + k], fw)
        d["m4_" + k] = O.consistency(d["bw_" + k], fw, frame)
    return d


# --------------------------------------------------------------------------------------------------------------------- GPU driver
def run_route(fav_amd, torch, net, d, route, sets):
    """one stream per option set: state from outside, one frame on `route`; returns [(in7, padded, mask)] as numpy arrays"""
    dev = torch.device("cuda", net.device)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    h, w = d["frame"].shape[:2]
    frame, state, fw, grey = T(d["frame"]), T(d["state"]), T(d["fw"]), T(d["grey"])
    bws = {"a": T(d["bw_a"]), "b": T(d["bw_b"])}
    torch.cuda.synchronize()               # (host-ordered look-ahead: the caller has seen the inputs complete)
    out = []
    for kind, border, inv, fix, fill, seed, r in sets:
        st = fav_amd.Stream(net, h, w, border=fav_amd.BORDER_CPU if border == "cpu" else fav_amd.BORDER_STN, min_filter_r=r,
                            invert_occlusion=bool(inv), fix_occlusions=bool(fix), fill_random=bool(fill), seed=seed)
        st.set_state(state)
        bw = bws[kind]
        if route == "cert":
            st.next_frame_cert(frame, bw, grey)
        elif route in ("flow3", "flow4", "two-launch"):
            st.next_frame_flow(frame, bw, fw, use_structure=(route == "flow4"))
        elif route in ("lookahead", "lookahead-host"):
            if route == "lookahead-host":
                st.set_host_ordered(True)
                torch.cuda.synchronize()
            st.prefetch_mask(frame, bw, fw, True)
            st.next_frame_flow(frame, bw, fw, use_structure=True)
        else:
            raise ValueError(route)
        out.append((st.last_input().cpu().numpy(), st.last_padded_input().cpu().numpy(), st.last_mask().cpu().numpy()))
        st.close()
    return out


# --------------------------------------------------------------------------------------------------------------------- CPU model
def f01(u8_hwc):
    return np.transpose(u8_hwc, (2, 0, 1)).astype(np.float32) / np.float32(255)


def model(O, d, mask_u8, opt):
    """the oracle's input of the frame a stream started with set_state assembles first (fill index 1), the certainty before the
    erosion with and without -fix_occlusions"""
    kind, border, inv, fix, fill, seed, r = opt
    bw = d["bw_" + kind]
    c01 = mask_u8.astype(np.float32) / np.float32(255)
    kw = dict(border=border, min_filter_r=r, invert_occlusion=bool(inv), fill_random=bool(fill), seed=seed, stn_f32=True)
    sty = O.Stylizer(None, fix_occlusions=bool(fix), **kw)
    sty.set_state(d["state"])
    with np.errstate(invalid="ignore", over="ignore"):
        x = sty.input7(f01(d["frame"]), bw, c01)
        cert = sty.certainty(bw, c01)
        unfixed = O.Stylizer(None, fix_occlusions=False, **kw).certainty(bw, c01)
    assert sty.count == 1
    return x, cert, unfixed


def same(a, b):
    """every value the same number, NaNs in the same places"""
    return np.array_equal(a, b, equal_nan=True)


if __name__ == "__main__":
    route, net_path, src, dst = sys.argv[1:5]
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.join(root, "fast-artistic-videos_amd", "python"))
    import torch
    import fav_amd
    data = dict(np.load(src, allow_pickle=False))
    sets = [(str(k), str(b), int(i), int(f), int(fl), int(s), int(r)) for k, b, i, f, fl, s, r in data.pop("sets")]
    res = run_route(fav_amd, torch, fav_amd.Net(net_path, 0), data, route, sets)
    np.savez(dst, **{f"{n}_{i}": a for i, t in enumerate(res) for n, a in zip(("in7", "pad", "mask"), t)})
