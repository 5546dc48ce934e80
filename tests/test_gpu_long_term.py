"""Long-term priors on the GPU: fav_long_term_input_f32 (csrc/kernels_longterm.hip) against the numpy model of
tests/util/long_term_model.py, its K = 1 identity with the stream's own input assembly, the stream entries (history, availability,
restart, flows given and estimated) and fav_stylize -long_term against a Python driver of the same library calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fav_amd import t7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import frame_input_model as M  # noqa: E402
import long_term_model as LT  # noqa: E402

pytestmark = pytest.mark.gpu
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
ONE_BLOCK_ARCH = "c9s1-8,d16,d32,R32,U2,c3s1-16,U2,c9s1-3"        # tiny_model.t7's layout with one residual block: padding 8
# (h, w, hs, ws): one ragged 64 x 16 tile | several tiles, H and W no multiples of 4, the state larger than the frame
SIZES = {"ragged": (17, 65, 20, 68), "state-larger": (53, 71, 56, 72)}
PAD = 16                                                          # tiny_model.t7's reflection padding


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def grey_certainties(h, w, K, seed):
    """K eroded-certainty planes in [0, 1]: grey values with patches of 0 and 1, so that every case of the weights occurs"""
    rng = np.random.default_rng(seed)
    c = rng.random((K, h, w)).astype(np.float32)
    c[:, :4] *= 0.3                                                # small values: c_k > used happens beyond distance 1
    for k in range(K):
        c[k, (2 * k + 5) % h] = 0.0
        c[k, (2 * k + 6) % h] = 1.0
    c[0, h // 2:h // 2 + 3, :w // 2] = 0.0                         # occluded at distance 1 ...
    if K > 1:
        c[1, h // 2:h // 2 + 3, :w // 4] = 1.0                     # ... visible at distance 2
    return c


@pytest.fixture(scope="module")
def op_inputs(oracle):
    """per size: frame, four states, four quantised flows (a seed each), computed once"""
    from fav_amd import synth
    out = {}
    for name, (h, w, hs, ws) in SIZES.items():
        rng = np.random.default_rng(900 + h)
        out[name] = dict(frame=synth.random_frame(h, w, 7), states=[(rng.standard_normal((3, hs, ws)) * 0.4 + 0.5).astype(np.float32) for _ in range(4)],
                         flows=[M.quantised_flow(h, w, 300 + 11 * k) for k in range(4)])
    return out


@pytest.mark.parametrize("size_name", list(SIZES))
@pytest.mark.parametrize("K", [1, 2, 4])
def test_operator_vs_model(favlib, oracle, cuda, op_inputs, size_name, K):
    h, w, hs, ws = SIZES[size_name]
    d = op_inputs[size_name]
    certs = grey_certainties(h, w, K, 50 + K)
    wts, _ = LT.weights(certs)
    assert (certs == 0).any() and (certs == 1).any() and (wts[0] == certs[0]).all()
    if K > 1:
        used = np.cumsum(certs, 0)[:-1]
        assert (certs[1:] <= used).any() and (certs[1:] > used).any() and (wts[1:] == 0).any() and (wts[1:] > 0).any()
    states, flows = d["states"][:K], d["flows"][:K]
    tol = 1e-5 * max(1.0, max(float(np.abs(s).max()) for s in states)) * 255
    frame01 = d["frame"].astype(np.float32) / np.float32(255)
    content = np.stack([frame01[..., 2 - c] * np.float32(255.0) - M.MEAN[c] for c in range(3)])
    gs, gf, gc, gframe = [T(s, cuda) for s in states], [T(f, cuda) for f in flows], [T(c, cuda) for c in certs], T(d["frame"], cuda)
    worst = 0.0
    for border in ("stn", "cpu"):
        for fill, seed, index in ((False, 0, 0), (True, 5, 3)):
            x, C = LT.merge_input(oracle, d["frame"], states, flows, list(certs), border, fill, seed, index)
            x64, _ = LT.merge_input(oracle, d["frame"], states, flows, list(certs), border, fill, seed, index, np.float64)
            assert np.abs(x[3:6] - x64[3:6]).max() <= tol                # the fp32 order of the model itself is within the bound
            for p in (PAD, 0):
                padded, cert_out = favlib.long_term_input(gframe, gs, gf, gc, border=favlib.BORDER_CPU if border == "cpu" else favlib.BORDER_STN,
                                                          pad=p, fill_random=fill, seed=seed, index=index)
                padded, cert_out = padded.cpu().numpy(), cert_out.cpu().numpy()
                interior = padded[p:p + h, p:p + w]
                in7 = np.transpose(interior[..., :7], (2, 0, 1))
                what = f"{size_name} K={K} {border} fill={fill} p={p}"
                assert np.array_equal(in7[:3], content), what + ": content"
                assert not padded[..., 7].any(), what + ": channel 7"
                assert np.array_equal(in7[6], C) and np.array_equal(cert_out, C), what + ": merged certainty"
                err = float(np.abs(in7[3:6] - x[3:6]).max())
                print(f"{what}: prior error {err:.3e} (bound {tol:.3e})")
                worst = max(worst, err)
                assert err <= tol, what
                assert np.array_equal(padded, np.pad(interior, ((p, p), (p, p), (0, 0)), mode="reflect")), what + ": padded ring"
    print(f"{size_name} K={K}: worst prior error {worst:.3e} (bound {tol:.3e})")


@pytest.mark.parametrize("fill", [False, True], ids=["vgg-mean", "uniform-random"])
def test_one_prior_is_the_streams_own_assembly(favlib, oracle, cuda, golden_dir, fill):
    """the operator with one distance writes the bytes of fav_stream_get_padded_input_f32 after fav_stream_next_frame_cert"""
    import torch
    net = favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)
    h, w = 53, 71
    ho, wo = net.output_size(h, w)
    d = M.make_inputs(oracle, h, w, ho, wo, 1040)
    for border in (favlib.BORDER_STN, favlib.BORDER_CPU):
        st = favlib.Stream(net, h, w, border=border, fill_random=fill, seed=5)
        st.set_state(T(d["state"], cuda))
        st.next_frame_cert(T(d["frame"], cuda), T(d["bw_a"], cuda), T(d["grey"], cuda))
        want = st.last_padded_input()
        cert = st.last_input()[6].contiguous()
        assert ((cert > 0) & (cert < 1)).any() and (cert == 0).any()
        got, C = favlib.long_term_input(T(d["frame"], cuda), [T(d["state"], cuda)], [T(d["bw_a"], cuda)], [cert], border=border,
                                        pad=net.input_pad(), fill_random=fill, seed=5, index=1)
        assert torch.equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} words differ"
        assert torch.equal(bits(C), bits(cert))
        st.close()


def test_wild_flow_of_an_unused_distance_leaves_nothing(favlib, oracle, cuda, op_inputs):
    import torch
    h, w, hs, ws = SIZES["state-larger"]
    d = op_inputs["state-larger"]
    wild = M.wild_flow(h, w, 77)
    certs = grey_certainties(h, w, 2, 9)
    certs[0, 0] = 1.0; certs[0, 5] = 1.0; certs[0, -1] = 1.0          # the rows of the non-finite and huge entries: distance 1 is certain
    wts, _ = LT.weights(certs)
    bad = ~np.isfinite(wild).all(-1) | (np.abs(wild) > 1e6).any(-1)
    assert bad.sum() >= 6 and not wts[1][bad].any() and (wts[1] > 0).any()
    args = (T(d["frame"], cuda), [T(s, cuda) for s in d["states"][:2]], [T(d["flows"][0], cuda), T(wild, cuda)], [T(c, cuda) for c in certs])
    a, _ = favlib.long_term_input(*args, pad=PAD)
    b, _ = favlib.long_term_input(*args, pad=PAD)
    assert torch.equal(bits(a), bits(b))
    in7 = np.transpose(a.cpu().numpy()[PAD:PAD + h, PAD:PAD + w, :7], (2, 0, 1))
    assert np.isfinite(in7[:, wts[1] == 0]).all(), "a prior of weight 0 left a non-finite value"
    x, _ = LT.merge_input(oracle, d["frame"], d["states"][:2], [d["flows"][0], wild], list(certs))
    tol = 1e-5 * max(1.0, max(float(np.abs(s).max()) for s in d["states"][:2])) * 255
    assert np.abs(in7[3:6][:, wts[1] == 0] - x[3:6][:, wts[1] == 0]).max() <= tol


# ------------------------------------------------------------------------------------------------------------------ the stream
@pytest.fixture(scope="module")
def scene(favlib, tmp_path_factory):
    d = tmp_path_factory.mktemp("long_term")
    path = str(d / "one_block.t7")
    t7.make_synthetic_checkpoint(path, arch=ONE_BLOCK_ARCH, seed=3)
    net = favlib.Net(path, 0)
    frames = [LT.scene_frame(i) for i in range(7)]
    yield d, path, net, frames
    net.close()


def test_stream_flows_given(favlib, oracle, cuda, scene):
    import torch
    _, _, net, frames = scene
    h, w, J = LT.SCENE_H, LT.SCENE_W, (1, 2, 4)
    st = favlib.Stream(net, h, w)
    st.set_long_term(J)
    assert st.long_term_available() == 0
    outs = [st.first_frame(T(frames[0], cuda))[0].cpu().numpy()]           # teacher forcing: the model's states are the GPU's own outputs
    tol = 1e-5 * 255
    seen, gained = [], 0
    for i in range(1, 7):
        seen.append(st.long_term_available())
        ds = [dd for dd in J if dd <= i]
        assert seen[-1] == len(ds)
        flows = [LT.scene_flows(i, dd) for dd in ds]
        bws, fws = [f[0] for f in flows], [f[1] for f in flows]
        out, _ = st.next_frame_flows_lt(T(frames[i], cuda), [T(b, cuda) for b in bws], [T(f, cuda) for f in fws])
        states = [outs[i - dd] for dd in ds]
        x, masks = LT.stream_input(oracle, frames[i], states, bws, fws)
        in7 = st.last_input().cpu().numpy()
        bound = tol * max(1.0, max(float(np.abs(s).max()) for s in states))
        assert np.array_equal(in7[:3], x[:3]) and np.array_equal(in7[6], x[6]), f"frame {i}"
        assert np.abs(in7[3:6] - x[3:6]).max() <= bound, f"frame {i}: {np.abs(in7[3:6] - x[3:6]).max():.3e} > {bound:.3e}"
        assert np.array_equal(st.last_mask().cpu().numpy(), masks[0]), "fav_stream_last_mask is not the distance-1 mask"
        if len(ds) > 1:
            c1 = oracle.min_filter(masks[0].astype(np.float32) / np.float32(255), 7)
            gained += int((x[6] > c1).sum())
        outs.append(out.cpu().numpy())
    assert seen == [1, 2, 2, 3, 3, 3] and gained > 0
    # more flows than the history serves, a null flow, a pending look-ahead: refused
    b, f = LT.scene_flows(6, 1)
    gb, gf, gfr = T(b, cuda), T(f, cuda), T(frames[6], cuda)
    st.first_frame(gfr)
    assert st.long_term_available() == 1
    with pytest.raises(favlib.FavError, match="serves 1"):
        st.next_frame_flows_lt(gfr, [gb, gb], [gf, gf])
    st.prefetch_mask(gfr, gb, gf)
    with pytest.raises(favlib.FavError, match="look-ahead"):
        st.next_frame_flows_lt(gfr, [gb], [gf])
    st.next_frame_flow(gfr, gb, gf)                                        # consumes the look-ahead, feeds the history
    assert st.long_term_available() == 2
    # a restart in the middle: the next frame's input is a fresh stream's
    st.first_frame(T(frames[3], cuda))
    assert st.long_term_available() == 1
    b4, f4 = LT.scene_flows(4, 1)
    st.next_frame_flows_lt(T(frames[4], cuda), [T(b4, cuda)], [T(f4, cuda)])
    fresh = favlib.Stream(net, h, w)
    fresh.set_long_term(J)
    fresh.first_frame(T(frames[3], cuda))
    fresh.next_frame_flows_lt(T(frames[4], cuda), [T(b4, cuda)], [T(f4, cuda)])
    assert torch.equal(bits(st.last_padded_input()), bits(fresh.last_padded_input()))
    st.close(); fresh.close()


def test_set_long_term_refusals(favlib, cuda, scene):
    _, _, net, _ = scene
    st = favlib.Stream(net, LT.SCENE_H, LT.SCENE_W)
    for bad, msg in (((2, 4), "must be 1"), ((1, 1), "ascending"), ((1, 4, 2), "ascending"), ((1, 17), "17"), ((1, 2, 3, 4, 5), "5 distances")):
        with pytest.raises(favlib.FavError, match=msg):
            st.set_long_term(bad)
    with pytest.raises(favlib.FavError, match="long-term priors are off"):
        st.long_term_workspace_bytes()
    st.close()


def test_off_means_off(favlib, cuda, scene):
    """J = {1} through the _lt entry is fav_stream_next_frame_estimate_ex3, byte for byte; after n = 0 the stream is an untouched one
    (the _lt entries, which take the previous frame from the history, are refused)"""
    import torch
    _, _, net, frames = scene
    g = [T(f, cuda) for f in frames[:4]]
    a, b = favlib.Stream(net, LT.SCENE_H, LT.SCENE_W), favlib.Stream(net, LT.SCENE_H, LT.SCENE_W)
    a.set_long_term((1,))
    a.first_frame(g[0]); b.first_frame(g[0])
    for use_structure, i in ((False, 1), (True, 2)):
        fa, ua, bwa, fwa = a.next_frame_estimate_lt(g[i], use_structure=use_structure, want_u8=True)
        fb, ub, bwb, fwb = b.next_frame_estimate(g[i], g[i - 1], use_structure=use_structure, want_u8=True, batched=True)
        assert torch.equal(bits(bwa[0]), bits(bwb)) and torch.equal(bits(fwa[0]), bits(fwb))
        assert torch.equal(a.last_mask(), b.last_mask())
        assert torch.equal(bits(a.last_padded_input()), bits(b.last_padded_input()))
        assert torch.equal(bits(fa), bits(fb)) and torch.equal(ua, ub)
    a.set_long_term(())
    with pytest.raises(favlib.FavError, match="long-term priors are off"):
        a.next_frame_estimate_lt(g[3])
    fa, ua, _, _ = a.next_frame_estimate(g[3], g[2], use_structure=True, want_u8=True, batched=True)
    fb, ub, _, _ = b.next_frame_estimate(g[3], g[2], use_structure=True, want_u8=True, batched=True)
    assert torch.equal(bits(fa), bits(fb)) and torch.equal(ua, ub)
    a.close(); b.close()


def test_estimate_path_flows_are_the_single_estimates(favlib, cuda, scene):
    import torch
    _, _, net, frames = scene
    g = [T(f, cuda) for f in frames[:4]]
    st = favlib.Stream(net, LT.SCENE_H, LT.SCENE_W)
    st.set_long_term((1, 2, 4))
    st.first_frame(g[0])
    nb = st.long_term_workspace_bytes()
    with pytest.raises(favlib.FavError, match="workspace"):
        st.next_frame_estimate_lt(g[1], workspace=torch.empty(nb - 256, dtype=torch.uint8, device=cuda))
    assert st.long_term_available() == 1                                  # the refused call left the history alone
    for i in (1, 2, 3):
        ds = [d for d in (1, 2, 4) if d <= i]
        _, _, bws, fws = st.next_frame_estimate_lt(g[i])
        assert len(bws) == len(ds)
        for k, d in enumerate(ds):
            assert torch.equal(bits(bws[k]), bits(favlib.flow_rgb8(g[i], g[i - d]))), f"frame {i}: backward flow of distance {d}"
            assert torch.equal(bits(fws[k]), bits(favlib.flow_rgb8(g[i - d], g[i]))), f"frame {i}: forward flow of distance {d}"
    st.close()


# ------------------------------------------------------------------------------------------------------------------ the CLI
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _write_clip(d, frames):
    import oracle as O
    d.mkdir()
    for i, f in enumerate(frames):
        O.write_pnm(str(d / f"frame_{i + 1:05d}.ppm"), f)


def _run(d, path, clip, out, *extra):
    r = subprocess.run([STYLIZE, "-input_pattern", str(d / clip / "frame_%05d.ppm"), "-output_prefix", str(d / out / "out"), "-model_vid", path,
                        "-model_img", "self", "-estimate_flow", "1", "-poll_settle", "0"] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def _driver(favlib, cuda, net, frames, J):
    """the frames fav_stylize writes, through the library calls (4-argument check: the program's default)"""
    st = favlib.Stream(net, LT.SCENE_H, LT.SCENE_W)
    if J:
        st.set_long_term(J)
    g = [T(f, cuda) for f in frames]
    out = [st.first_frame(g[0], want_f32=False, want_u8=True)[1].cpu().numpy()]
    for i in range(1, len(g)):
        u = st.next_frame_estimate_lt(g[i], use_structure=True, want_f32=False, want_u8=True)[1] if J else \
            st.next_frame_estimate(g[i], g[i - 1], use_structure=True, want_f32=False, want_u8=True, batched=True)[1]
        out.append(u.cpu().numpy())
    st.close()
    return out


def test_cli(favlib, cuda, scene):
    d, path, net, frames = scene
    clip = frames[1:6]
    _write_clip(d / "clip", clip)
    _run(d, path, "clip", "lt", "-long_term", "2")
    _run(d, path, "clip", "plain")
    want_lt, want_plain = _driver(favlib, cuda, net, clip, (1, 2)), _driver(favlib, cuda, net, clip, ())
    for k in range(5):
        assert np.array_equal(_png(d / "lt" / f"out-{k + 1:05d}.png"), want_lt[k]), f"-long_term 2: frame {k + 1}"
        assert np.array_equal(_png(d / "plain" / f"out-{k + 1:05d}.png"), want_plain[k]), f"without the flag: frame {k + 1}"
    assert any(not np.array_equal(want_lt[k], want_plain[k]) for k in range(2, 5)), "the long-term priors change no frame of this clip"
    # a hard cut at frame 3: the history restarts there, frame 4 is the second frame of a clip that starts at frame 3
    cut = [f // 2 for f in clip[:2]] + [255 - f // 2 for f in clip[2:]]
    _write_clip(d / "cutclip", cut)
    _write_clip(d / "tail", cut[2:])
    r = _run(d, path, "cutclip", "cut", "-long_term", "2", "-scene_cut", "0.5", "-scene_cut_log", str(d / "cut" / "log.txt"))
    _run(d, path, "tail", "tailout", "-long_term", "2")
    log = [ln.split() for ln in open(d / "cut" / "log.txt").read().splitlines()]
    assert [int(row[3]) for row in log] == [0, 0, 1, 0, 0], log
    assert r.stdout.count("stylizing frame independently") == 2
    for k in (1, 2, 3):
        assert open(d / "cut" / f"out-{k + 2:05d}.png", "rb").read() == open(d / "tailout" / f"out-{k:05d}.png", "rb").read(), f"frame {k + 2}"
