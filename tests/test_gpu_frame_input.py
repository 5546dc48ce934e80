"""The network input of a frame -- the eight floats per pixel that min_filter_kernel<1|2> + prep_input_kernel and check_prep_kernel
(csrc/kernels_frame.hip) write -- read back channel by channel, padded ring included, on every route of the stream and compared with
the CPU oracle: fp32 restatements that share no code with the kernels (oracle.warp "stn_f32" / "cpu", min_filter, assemble,
consistency, fill_uniform and the option arithmetic of Stylizer.certainty).

Routes   cert (mask file), flow3 / flow4 (the fused check_prep_kernel in the checker's 3- and 4-argument mode), lookahead
         (prefetch_mask in the 4-argument mode, event-ordered at every size and host-ordered at one), two-launch (a child process on
         the diagnostic library with FAV_NO_CHECK_PREP=1: min_filter_kernel<2> + prep_input_kernel, 3-argument mode).
Sizes    smallest      (p + 1, p + 1) = 17 x 17 with tiny_model.t7's padding p = 16: the smallest frame a stream accepts
         one-tile      16 x 64, exactly one 64 x 16 tile.  tiny_model.t7 cannot run it (16 rows are not more than its padding of 16),
                       so this size alone runs a synthetic model of the same layout with ONE residual block, whose padding is 8
         ragged        17 x 65: one-pixel ragged tiles on both axes
         seams         33 x 130: interior tile seams on both axes
         state-larger  53 x 71: the state is 56 x 72, the prior is sampled with the state's bounds and pitch
Options  border stn | cpu, invert_occlusion, fix_occlusions, fill vgg-mean | uniform-random (two seeds), window r in {1, 2, 7, 8, 15}
         -- all of them at every (route, size): flow (a) under both borders and flow (b) under the STN border, 180 streams per case.
Inputs   tests/util/frame_input_model.py: an unclamped random state set with set_state; grey mask bytes with zeros on the tile seams,
         in the corners and on the edges; flow (a) on the grid of multiples of 1/8 (every bilinear weight and sum of weights exact in
         fp32, so the all-ones warp of -fix_occlusions and with it the whole certainty channel is the same number in any order) with a
         band that leaves the image by exactly half a pixel and one that leaves it entirely; flow (b) unrestricted, with NaN, +-inf,
         2^31, -3e9 and 1e20.

What keeps the comparisons from being vacuous is asserted as well.  Two of those guards can hold on the mask-file route only and are
asserted there: the checker's bytes are 0 and 255, so only the grey mask puts values strictly between 0 and 1 into channel 6; and the
checker already marks every pixel whose flow leaves the image as unreliable, so on the flow routes -fix_occlusions finds certainty to
remove only under -invert_occlusion, where a pixel it keeps need not exist in a 17 x 17 frame.  On the flow routes the mask must hold
both bytes instead."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from fav_amd import t7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import frame_input_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DIAG_LIB = os.path.join(ROOT, "fast-artistic-videos_amd", "libfav_diag.so")
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
SIZES = {"smallest": None, "one-tile": (16, 64), "ragged": (17, 65), "seams": (33, 130), "state-larger": (53, 71)}
# seeds of the inputs, per size.  The smallest one is chosen so that the widest window still leaves a grey certainty at the centre of
# the 17 x 17 frame under every option (the 15 x 15 bytes around it hold neither 0 nor 255): the test asserts that it does
SEEDS = {"smallest": 2110, "one-tile": 1010, "ragged": 1020, "seams": 1030, "state-larger": 1040}
ONE_BLOCK_ARCH = "c9s1-8,d16,d32,R32,U2,c3s1-16,U2,c9s1-3"        # tiny_model.t7's layout with one residual block: padding 8
CASES = [(r, s) for s in SIZES for r in M.ROUTES if r != "lookahead-host"] + [("lookahead-host", "ragged")]


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def setup(favlib, oracle, cuda, golden_dir, tmp_path_factory):
    """per size, built once and shared by the routes: (h, w, p, model file, Net, inputs); the oracle's inputs per (size, mask, options)"""
    tiny = os.path.join(golden_dir, "tiny_model.t7")
    one_block = str(tmp_path_factory.mktemp("frame_input") / "one_block.t7")
    t7.make_synthetic_checkpoint(one_block, arch=ONE_BLOCK_ARCH, seed=3)
    nets, sizes, models = {}, {}, {}

    def size(name):
        if name not in sizes:
            path = one_block if name == "one-tile" else tiny
            if path not in nets:
                nets[path] = favlib.Net(path, 0)
            net = nets[path]
            p = net.input_pad()
            h, w = SIZES[name] or (p + 1, p + 1)
            ho, wo = net.output_size(h, w)
            d = M.make_inputs(oracle, h, w, ho, wo, SEEDS[name])
            # the inputs reach what they were made for: the all-ones warp is exactly 0.5 somewhere (sign 0) and 0 elsewhere under the STN
            # border, the flow routes' masks hold both bytes, the state leaves [0, 1]
            ones = oracle.warp(np.ones((1, h, w), np.float32), oracle.flo_to_lua(d["bw_a"]), "stn_f32")[0]
            assert (ones == 0.5).any() and (ones == 0).any() and (ones == 1).any()
            for k in ("m3_a", "m4_a", "m3_b", "m4_b"):
                assert d[k].min() == 0 and d[k].max() == 255, k
            assert d["state"].min() < 0 and d["state"].max() > 1 and (d["grey"] == 0).any() and len(np.unique(d["grey"])) > 100
            sizes[name] = (h, w, p, path, net, d)
        return sizes[name]

    def model(name, mask_name, opt):
        key = (name, mask_name, opt)
        if key not in models:
            d = size(name)[5]
            models[key] = M.model(oracle, d, d["grey"] if mask_name == "grey" else d[mask_name + "_" + opt[0]], opt)
        return models[key]

    yield size, model
    models.clear(); sizes.clear(); nets.clear()


def _ring_and_interior(padded, in7, h, w, p):
    """channel 7 is zero, the interior of the padded view is last_input(), the ring is numpy's reflection of that interior"""
    assert padded.shape == (h + 2 * p, w + 2 * p, 8)
    interior = padded[p:p + h, p:p + w]
    assert M.same(np.transpose(interior[..., :7], (2, 0, 1)), in7), "interior of the padded view differs from last_input()"
    assert not padded[..., 7].any(), "channel 7 is not zero"
    want = np.pad(interior, ((p, p), (p, p), (0, 0)), mode="reflect")
    assert M.same(padded, want), f"{(~((padded == want) | (np.isnan(padded) & np.isnan(want)))).sum()} floats of the padded ring differ"


@pytest.mark.parametrize("route,size_name", CASES, ids=[f"{r}-{s}" for r, s in CASES])
def test_frame_input_vs_model(favlib, oracle, cuda, setup, tmp_path, route, size_name):
    import torch
    size, model = setup
    h, w, p, path, net, d = size(size_name)
    sets = M.option_sets(M.R_ALL)
    t0 = time.perf_counter()
    if route == "two-launch":
        np.savez(tmp_path / "in.npz", sets=np.array([[str(v) for v in s] for s in sets]), **d)
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "util", "frame_input_model.py"), route, path,
                               str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                              env=dict(os.environ, FAV_AMD_LIB=DIAG_LIB, FAV_NO_CHECK_PREP="1"), timeout=300)
        z = np.load(tmp_path / "out.npz")
        results = [(z[f"in7_{i}"], z[f"pad_{i}"], z[f"mask_{i}"]) for i in range(len(sets))]
    else:
        results = M.run_route(favlib, torch, net, d, route, sets)
    t_gpu = time.perf_counter() - t0
    mask_name = M.MASK_OF[route]
    frame01 = d["frame"].astype(np.float32) / np.float32(255)
    content = np.stack([frame01[..., 2 - c] * np.float32(255.0) - M.MEAN[c] for c in range(3)])      # the existing test's expression
    tol = 1e-5 * max(1.0, float(np.abs(d["state"]).max())) * 255            # test_warp_matches_oracle's bound through the pre-processing
    worst, priors = 0.0, {}
    for opt, (in7, padded, mask) in zip(sets, results):
        kind, border, inv, fix, fill, seed, r = opt
        mask_u8 = d["grey"] if mask_name == "grey" else d[mask_name + "_" + kind]
        assert np.array_equal(mask, mask_u8), f"{opt}: {(mask != mask_u8).sum()} mask bytes differ from the oracle"
        x, cert, unfixed = model(size_name, mask_name, opt)
        assert np.array_equal(in7[:3], content), f"{opt}: content channels"
        want6 = oracle.min_filter(cert, r)
        assert M.same(x[6], want6)
        assert M.same(in7[6], want6), f"{opt}: {(in7[6] != want6).sum()} certainties differ, worst {np.abs(in7[6] - want6).max():.3e}"
        if route == "cert":
            # (flow (b) moves every pixel by some four pixels in a random direction: under -fix_occlusions no wide window of a 17-row
            # frame is without a pixel that left the image, so the grey guard is flow (a)'s, the flow whose arithmetic is exact)
            assert kind == "b" or ((want6 > 0) & (want6 < 1)).any(), f"{opt}: no grey value left in channel 6"
            if fix:
                assert ((unfixed > 0) & (cert == 0)).any() and ((unfixed > 0) & (cert > 0)).any(), f"{opt}: -fix_occlusions removes or keeps nothing"
        if border == "stn":
            bad = ~((in7[3:6] == x[3:6]) | (np.isnan(in7[3:6]) & np.isnan(x[3:6])))
            assert not bad.any(), f"{opt}: {bad.sum()} prior values differ"
            assert kind == "a" or np.isnan(x[3:6]).any()
        else:
            err = float(np.abs(in7[3:6] - x[3:6]).max())
            worst = max(worst, err)
            assert err <= tol, f"{opt}: CPU-border prior error {err:.3e} > {tol:.3e}"
        priors[opt] = x[3:6]
        _ring_and_interior(padded, in7, h, w, p)
    # the two seeds of the uniform-random fill give two priors, and both differ from the vgg-mean one
    for (kind, border, inv, fix, fill, seed, r), x in priors.items():
        if fill and seed == M.FILLS[1][1]:
            for other in (M.FILLS[0], M.FILLS[2]):
                assert not M.same(x, priors[(kind, border, inv, fix) + other + (r,)])
    print(f"{route} {h}x{w} (p = {p}): {len(sets)} option sets, GPU part {t_gpu:.2f} s, worst CPU-border prior error {worst:.3e} (bound {tol:.3e})")


@pytest.mark.parametrize("fill,seed", [(False, 1), (True, 5)], ids=["vgg-mean", "uniform-random"])
def test_first_frame_input_and_fill_index(favlib, oracle, cuda, setup, fill, seed):
    """a stream's first frame has no prior: channels 3..5 are the fill alone (zero | the counter RNG with index 1), channel 6 is zero.
    The frame after it is assembled with index 2; after set_state instead of a first frame, with index 1 (fav_stream::frame_counter
    counts assembled frames, and set_state assembles none)."""
    size, _ = setup
    h, w, p, path, net, d = size("ragged")
    f01 = M.f01(d["frame"])
    st = favlib.Stream(net, h, w, fill_random=fill, seed=seed)
    ref = oracle.Stylizer(None, fill_random=fill, seed=seed, stn_f32=True)
    st.first_frame(T(d["frame"], cuda))
    in7, padded = st.last_input().cpu().numpy(), st.last_padded_input().cpu().numpy()
    x = ref.first_input7(f01)
    assert ref.count == 1 and np.array_equal(in7, x) and not in7[6].any()
    assert bool(in7[3:6].any()) == fill
    _ring_and_interior(padded, in7, h, w, p)
    state = st.state().cpu().numpy()
    ref.set_state(state)
    st.next_frame_cert(T(d["frame"], cuda), T(d["bw_a"], cuda), T(d["grey"], cuda))
    second = st.last_input().cpu().numpy()
    x2 = ref.input7(f01, d["bw_a"], d["grey"].astype(np.float32) / np.float32(255))
    assert ref.count == 2 and M.same(second, x2)
    st2 = favlib.Stream(net, h, w, fill_random=fill, seed=seed)
    st2.set_state(T(state, cuda))
    st2.next_frame_cert(T(d["frame"], cuda), T(d["bw_a"], cuda), T(d["grey"], cuda))
    ref2 = oracle.Stylizer(None, fill_random=fill, seed=seed, stn_f32=True)
    ref2.set_state(state)
    x1 = ref2.input7(f01, d["bw_a"], d["grey"].astype(np.float32) / np.float32(255))
    assert ref2.count == 1 and M.same(st2.last_input().cpu().numpy(), x1)
    assert M.same(x1, x2) != fill                # the index is part of the fill's key


def test_window_above_the_limit_is_refused_at_create(favlib, oracle, cuda, setup):
    """-occlusions_min_filter 16 exceeds the erosion kernels' LDS tiles (1..15): the stream and the VR pipeline refuse it when they are
    created, not at the second frame; r <= 0 keeps its clamp to 1; the operator's own check is still there"""
    size, _ = setup
    h, w, p, path, net, d = size("ragged")
    for r in (16, 17, 1 << 20):
        with pytest.raises(favlib.FavError, match="occlusions_min_filter.*15"):
            favlib.Stream(net, h, w, min_filter_r=r)
    with pytest.raises(favlib.FavError, match="occlusions_min_filter 16.*15"):
        favlib.VR(net, 64, 64, min_filter_r=16)
    with pytest.raises(favlib.FavError, match=r"window 16 unsupported \(1\.\.15\)"):
        favlib.min_filter(T(np.ones((h, w), np.float32), cuda), 16)
    # r = 0 and r = -3 run as r = 1, the one-pixel window
    c01 = d["grey"].astype(np.float32) / np.float32(255)
    for r in (0, -3, 15):
        st = favlib.Stream(net, h, w, min_filter_r=r)
        st.set_state(T(d["state"], cuda))
        st.next_frame_cert(T(d["frame"], cuda), T(d["bw_a"], cuda), T(d["grey"], cuda))
        assert np.array_equal(st.last_input().cpu().numpy()[6], oracle.min_filter(c01, max(r, 1)))


def test_fav_stylize_refuses_the_window_before_writing(favlib, oracle, tmp_path, golden_dir):
    """fav_stylize -occlusions_min_filter 16 used to write frame 1 and fail at frame 2; now it exits non-zero with no output file"""
    from fav_amd import synth
    h, w = 48, 64
    os.makedirs(tmp_path / "flow"); os.makedirs(tmp_path / "out")
    for i in (1, 2):
        oracle.write_pnm(str(tmp_path / f"frame_{i:05d}.ppm"), synth.smooth_frame(h, w, i))
    bw = synth.backward_flow(h, w, 3)
    oracle.write_flo(str(tmp_path / "flow" / "backward_2_1.flo"), bw)
    oracle.write_flo(str(tmp_path / "flow" / "forward_1_2.flo"), synth.forward_flow_from_backward(bw, 4))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import e2e_content
    e2e_content.age_files(str(tmp_path))           # finished inputs say so through their modification time (host/fav_poll.h)
    cmd = [os.path.join(BIN, "fav_stylize"), "-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-flow_pattern", str(tmp_path / "flow" / "backward_[%d]_{%d}.flo"),
           "-forward_flow_pattern", str(tmp_path / "flow" / "forward_{%d}_[%d].flo"), "-structure", "0", "-output_prefix", str(tmp_path / "out" / "out"), "-gpu", "0",
           "-model_vid", os.path.join(golden_dir, "tiny_model.t7"), "-model_img", "self"]
    r = subprocess.run(cmd + ["-occlusions_min_filter", "16"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "occlusions_min_filter 16" in r.stderr and "15" in r.stderr, (r.returncode, r.stderr)
    assert os.listdir(tmp_path / "out") == []
    r = subprocess.run(cmd + ["-occlusions_min_filter", "15"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and sorted(os.listdir(tmp_path / "out")) == ["out-00001.png", "out-00002.png"], r.stderr
