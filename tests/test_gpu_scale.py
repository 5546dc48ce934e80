"""-scale_factor on the GPU (-m gpu): the bicubic resampling kernels (csrc/kernels_scale.hip) against the numpy restatement of
image.scale(.., 'bicubic') (tests/util/bicubic_model.py), and the scaled single-image path of the stream and of fav_stylize against the
composition  scale(oracle first frame(scale(frame, Hs, Ws)), H, W)  (fast_artistic_video_core.lua:127-130,146,150-152).

Tolerances:
  * operator: with e32 = max|M32 - M64| of the two CPU models on the same input, max|GPU - M64| <= max(4 e32, 2^-22 max|src|) -- the
    factor 4 lets the compiler contract a*b+c and the two passes compound; nothing is measured against the code under test;
  * stream: 2e-4 (the project's first-frame tolerance, test_gpu_parity.py) x 25/16 (the L1 gain of the separable kernel: 1 + x - x^2
    peaks at 5/4 per axis) plus the operator bound for the way back; PNGs within 1 LSB of the oracle's quantisation (the CLI tolerance).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from fav_amd import synth, t7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import bicubic_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
VID = os.path.join(ROOT, "tests", "golden", "tiny_model.t7")
IMG_ARCH = "c9s1-8,d16,d32,R32,R32,u16,u8,c9s1-3"       # (test_image_model_vs_oracle's image model)
FIRST_TOL = 2e-4
EUNSUPPORTED, EINVAL = "libfav error -4", "libfav error -1"


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _f01(u8):
    return np.transpose(u8, (2, 0, 1)).astype(np.float32) / np.float32(255)


def _layers(path):
    return t7.extract_layers(t7.load(path)["model"])


def operator_bound(src, hd, wd):
    """(bound, M64) for resampling src to hd x wd"""
    m64 = M.scale(src, hd, wd, np.float64)
    e32 = np.abs(M.scale(src, hd, wd, np.float32).astype(np.float64) - m64).max()
    return max(4 * e32, 2.0 ** -22 * float(np.abs(src).max())), m64


@functools.lru_cache(maxsize=None)
def _clip(h, w):
    """three frames with the flows and 3-argument masks between them (computed once per size)"""
    import oracle as O
    frames = [synth.smooth_frame(h, w, 300 + i) for i in range(3)]
    bws = [None] + [synth.backward_flow(h, w, 400 + i) for i in range(1, 3)]
    fws = [None] + [synth.forward_flow_from_backward(bws[i], 500 + i) for i in range(1, 3)]
    masks = [None] + [O.consistency(bws[i], fws[i]) for i in range(1, 3)]
    return frames, bws, fws, masks


@functools.lru_cache(maxsize=None)
def _image_model(tmp):
    p = os.path.join(tmp, "img.t7")
    t7.make_synthetic_checkpoint(p, arch=IMG_ARCH, seed=5, in_channels=3, use_instance_norm=True)
    return p


@functools.lru_cache(maxsize=None)
def _composition(h, w, hs, ws, k, image_model=None):
    """(expected [3][h][w], bound) of frame k of _clip(h, w) stylised at hs x ws by the oracle and scaled back"""
    import oracle as O
    ref = O.Stylizer(_layers(VID))
    small = ref.first(M.scale(_f01(_clip(h, w)[0][k]), hs, ws, np.float32), image_layers=_layers(image_model) if image_model else None)
    assert small.shape == (3, hs, ws)
    bound, _ = operator_bound(small, h, w)
    out = M.scale(small, h, w, np.float32)
    out.setflags(write=False)
    return out, FIRST_TOL * 25 / 16 + bound


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("scale_models"))


# ---------------------------------------------------------------------------------------------- 1. the operator
@pytest.mark.parametrize("k", range(len(M.CASES)), ids=["%dx%dx%d-%dx%d" % c for c in M.CASES])
def test_scale_bicubic_matches_the_model(favlib, cuda, k):
    c, hs, ws, hd, wd = M.CASES[k]
    for src in M.case_inputs(k):
        got = favlib.scale_bicubic(T(src, cuda), hd, wd).cpu().numpy()
        assert got.shape == (c, hd, wd)
        bound, m64 = operator_bound(src, hd, wd)
        err = np.abs(got.astype(np.float64) - m64).max()
        print(f"case {M.CASES[k]} max|src| {np.abs(src).max():.4g}: max|GPU - M64| = {err:.3e}, bound {bound:.3e}, "
              f"max|GPU - M32| = {np.abs(got - M.scale(src, hd, wd, np.float32)).max():.3e}")
        assert err <= bound
        # exact, whatever the arithmetic: an axis of equal length is copied, the last sample is the source's
        if hd == hs: assert np.array_equal(got[:, :, -1], src[:, :, -1])
        if wd == ws: assert np.array_equal(got[:, -1, :], src[:, -1, :])
        if wd == ws and hs == 1: assert np.array_equal(got, np.repeat(src, hd, axis=1))      # the one-row source repeated, its width copied
        assert np.array_equal(got[:, -1, -1], src[:, -1, -1])
    same = M.case_inputs(k)[0]
    assert np.array_equal(favlib.scale_bicubic(T(same, cuda), hs, ws).cpu().numpy(), same)      # both axes equal: the copy


# ---------------------------------------------------------------------------------------------- 2. / 3. the stream
def _run_stream(favlib, oracle, cuda, h, w, hs, ws, image_model):
    frames, bws, fws, masks = _clip(h, w)
    net = favlib.Net(VID, 0)
    st = favlib.Stream(net, h, w)
    if image_model:
        net_img = favlib.Net(image_model, 0)
        st.set_image_net(net_img)
    st.set_single_image_size(hs, ws)
    o0, u0 = st.first_frame(T(frames[0], cuda), want_u8=True)
    o0 = o0.cpu().numpy()
    want, tol = _composition(h, w, hs, ws, 0, image_model)
    err = np.abs(o0 - want).max()
    print(f"{h}x{w} at {hs}x{ws} ({'image' if image_model else 'video'} model): max|GPU - composition| = {err:.3e}, bound {tol:.3e}")
    assert o0.shape == (3, h, w) and err <= tol
    assert np.array_equal(u0.cpu().numpy(), oracle.to_u8_hwc(o0))            # image.save's quantisation of the float frame
    assert np.array_equal(st.state().cpu().numpy(), o0)                      # the state landed at H x W
    # the next frame at full size, teacher-forced: the arena came back to H x W
    o1, _ = st.next_frame_flow(T(frames[1], cuda), T(bws[1], cuda), T(fws[1], cuda))
    ref = oracle.Stylizer(_layers(VID)); ref.last = o0
    r1 = ref.next(_f01(frames[1]), bws[1], masks[1].astype(np.float32) / np.float32(255))
    err1 = np.abs(o1.cpu().numpy() - r1).max()
    print(f"  next frame at {h}x{w}: max|GPU - oracle| = {err1:.3e}")
    assert err1 <= FIRST_TOL
    net.check()


def test_stream_scaled_first_frame_video_model(favlib, oracle, cuda):
    _run_stream(favlib, oracle, cuda, 96, 128, 48, 64, None)


@pytest.mark.parametrize("geom", [(96, 128, 48, 64), (64, 96, 48, 72), (48, 64, 72, 96)], ids=["half", "three-quarters", "up-1.5"])
def test_stream_scaled_first_frame_image_model(favlib, oracle, cuda, model_dir, geom):
    _run_stream(favlib, oracle, cuda, *geom, _image_model(model_dir))


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_set_single_image_size_refusals(favlib, cuda):
    net = favlib.Net(VID, 0)
    odd = favlib.Stream(net, 50, 70)                                   # stylised frames are 52x72: nothing to scale back to
    assert (odd.Ho, odd.Wo) != (50, 70)
    with pytest.raises(favlib.FavError, match=EUNSUPPORTED):
        odd.set_single_image_size(24, 32)
    first = _layers(VID)[0]
    assert first["type"] == "pad" and first["l"] > 0
    st = favlib.Stream(net, 96, 128)
    for hs, ws in [(first["l"], 64), (48, first["l"]), (0, 64), (-4, -4)]:
        with pytest.raises(favlib.FavError, match=EINVAL):
            st.set_single_image_size(hs, ws)
    # 0, 0 restores the plain path: the same bits as a stream that never had a scaled size
    frame = T(_clip(96, 128)[0][0], cuda)
    st.set_single_image_size(48, 64)
    scaled, _ = st.first_frame(frame)
    st.set_single_image_size(0, 0)
    back, _ = st.first_frame(frame)
    plain, _ = favlib.Stream(net, 96, 128).first_frame(frame)
    assert np.array_equal(back.cpu().numpy(), plain.cpu().numpy())
    assert not np.array_equal(scaled.cpu().numpy(), plain.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 5. the CLI
def _write_inputs(oracle, d, h, w, n):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import e2e_content
    frames, bws, fws, masks = _clip(h, w)
    os.makedirs(d / "flow", exist_ok=True)
    for i in range(1, n + 1):
        oracle.write_pnm(str(d / f"frame_{i:05d}.ppm"), frames[i - 1])
        if i > 1:
            oracle.write_flo(str(d / "flow" / f"backward_{i}_{i-1}.flo"), bws[i - 1])
            oracle.write_pnm(str(d / "flow" / f"reliable_{i}_{i-1}.pgm"), masks[i - 1])
    e2e_content.age_files(str(d))          # finished inputs say so through their modification time (host/fav_poll.h)
    return [os.path.join(BIN, "fav_stylize"), "-input_pattern", str(d / "frame_%05d.ppm"), "-output_prefix", str(d / "out" / "out"), "-gpu", "0",
            "-model_vid", VID, "-model_img", "self"]


def _png(d, i):
    from PIL import Image
    return np.asarray(Image.open(str(d / "out" / f"out-{i:05d}.png")))


def test_fav_stylize_scale_factor_create_inconsistent(oracle, favlib, tmp_path):
    h, w, n = 96, 128, 3
    cmd = _write_inputs(oracle, tmp_path, h, w, n)
    r = subprocess.run(cmd + ["-create_inconsistent", "-scale_factor", "0.5"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("Writing output image to") == n, r.stderr
    for i in range(1, n + 1):
        png = _png(tmp_path, i)
        want = oracle.to_u8_hwc(_composition(h, w, 48, 64, i - 1)[0])
        assert png.shape == (h, w, 3)
        assert np.abs(png.astype(int) - want.astype(int)).max() <= 1, f"frame {i}"


def test_fav_stylize_scale_factor_then_full_size_frames(oracle, favlib, tmp_path):
    h, w, n = 96, 128, 2
    frames, bws, fws, masks = _clip(h, w)
    cmd = _write_inputs(oracle, tmp_path, h, w, n) + ["-flow_pattern", str(tmp_path / "flow" / "backward_[%d]_{%d}.flo"),
                                                     "-occlusions_pattern", str(tmp_path / "flow" / "reliable_[%d]_{%d}.pgm")]
    r = subprocess.run(cmd + ["-scale_factor", "0.5"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("Writing output image to") == n, r.stderr
    first = _composition(h, w, 48, 64, 0)[0]
    assert np.abs(_png(tmp_path, 1).astype(int) - oracle.to_u8_hwc(first).astype(int)).max() <= 1      # frame 1 is scaled
    ref = oracle.Stylizer(_layers(VID)); ref.last = np.array(first)                 # ... and the oracle's chain goes on from ITS frame 1
    second = ref.next(_f01(frames[1]), bws[1], masks[1].astype(np.float32) / np.float32(255))
    assert np.abs(_png(tmp_path, 2).astype(int) - oracle.to_u8_hwc(second).astype(int)).max() <= 1
    # 96 * 0.3 = 28.8: img:view(1, 3, H * f, W * f) has no such size
    r = subprocess.run(cmd + ["-scale_factor", "0.3"], capture_output=True, text=True)
    assert r.returncode != 0 and "-scale_factor" in r.stderr and "128x96" in r.stderr, (r.returncode, r.stderr)
