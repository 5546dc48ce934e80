"""-original_colors on the GPU: fav_color_transfer_rgb8 / _yuv byte-equal to the fp32 numpy model (tests/util/color_model.py) over odd
sizes, tails and all twelve formats, written completely and nowhere else; the planes operator against the composition of the image
operator with fav_rgb8_to_yuv; the stream forms, which must not touch the state; and fav_stylize -original_colors 1 through its three
sinks against the model applied to the frames of the run without the flag."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import color_model as CM  # noqa: E402
import scene_model as S  # noqa: E402
import yuv_model as M  # noqa: E402

from fav_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
# (W, H): one pixel; one 4:2:0 sample; an odd edge in each direction; full lane blocks (8 x 2 pixels) only; a tail narrower than a
# block behind full ones, more than one workgroup (256 lanes); a row of 32 full blocks and a 2-column tail
SIZES = [(1, 1), (2, 2), (5, 3), (17, 9), (64, 48), (131, 67), (258, 6)]
MATRICES = ["601", "709"]
GUARD, PATTERN = 64, 0xA5


def _cfmt(favlib, f):
    return favlib.yuv_format(favlib.YUV_444 if f.chroma == "444" else favlib.YUV_420,
                             favlib.YUV_SITING_LEFT if f.siting == "left" else favlib.YUV_SITING_CENTER,
                             favlib.YUV_BT709 if f.matrix == "709" else favlib.YUV_BT601, f.full_range)


def _cmatrix(favlib, m):
    return favlib.YUV_BT709 if m == "709" else favlib.YUV_BT601


def _inputs(w, h):
    """the state: values below 0, above 1, exactly k/255 and one ulp below k/255 (image.save truncates: the byte changes there);
    the original: random bytes salted with 0 / 1 / 254 / 255 so that the result clamps at both ends"""
    rng = np.random.default_rng(7000 * w + h)
    st = rng.uniform(-0.3, 1.3, (3, h, w)).astype(np.float32)
    pick = rng.random((3, h, w))
    k = (rng.integers(0, 256, (3, h, w)).astype(np.float32) / np.float32(255))
    st = np.where(pick < 0.25, k, st)
    st = np.where((pick >= 0.25) & (pick < 0.5), np.nextafter(k, np.float32(0)), st).astype(np.float32)
    orig = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    flat = orig.reshape(-1)
    n = max(2, flat.size // 4)
    flat[rng.integers(0, flat.size, n)] = rng.choice(np.array([0, 1, 254, 255], np.uint8), n)
    return np.ascontiguousarray(st), orig


@pytest.fixture(scope="module")
def cases():
    """inputs and the model's outputs for every size, matrix and format, computed once"""
    out = {}
    for w, h in SIZES:
        st, orig = _inputs(w, h)
        P = {m: CM.transfer(st, orig, m) for m in MATRICES}
        out[(w, h)] = dict(state=st, orig=orig, P=P, planes={f: M.rgb_to_yuv(P[f.matrix], f) for f in M.ALL_FORMATS})
    return out


def _guarded(torch, cuda, n):
    return torch.full((n + GUARD,), PATTERN, dtype=torch.uint8, device=cuda)


def _check_written(buf, n, want, what):
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n], want.reshape(-1)), f"{what}: {int((got[:n] != want.reshape(-1)).sum())} of {n} bytes differ from the model"
    assert (got[n:] == PATTERN).all(), f"{what}: bytes behind the output were written"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_operators_equal_the_fp32_model_byte_for_byte(favlib, cuda, cases, size):
    import torch
    w, h = size
    c = cases[size]
    if w * h >= 64:                                            # the inputs do what they are meant to: both clamps happen
        assert (c["P"]["601"] == 0).any() and (c["P"]["601"] == 255).any()
    st, orig = torch.from_numpy(c["state"]).to(cuda), torch.from_numpy(c["orig"]).to(cuda)
    for m in MATRICES:
        a, b = _guarded(torch, cuda, h * w * 3), _guarded(torch, cuda, h * w * 3)
        favlib.color_transfer(st, orig, _cmatrix(favlib, m), out=a); favlib.color_transfer(st, orig, _cmatrix(favlib, m), out=b)
        _check_written(a, h * w * 3, c["P"][m], f"fav_color_transfer_rgb8 {w}x{h} BT.{m}")
        assert torch.equal(a, b), f"fav_color_transfer_rgb8 {w}x{h} BT.{m}: two calls differ"
    for f in M.ALL_FORMATS:
        n = M.frame_bytes(w, h, f)
        a, b = _guarded(torch, cuda, n), _guarded(torch, cuda, n)
        favlib.color_transfer(st, orig, _cfmt(favlib, f), out=a); favlib.color_transfer(st, orig, _cfmt(favlib, f), out=b)
        _check_written(a, n, c["planes"][f], f"fav_color_transfer_yuv {w}x{h} {f}")
        assert torch.equal(a, b), f"fav_color_transfer_yuv {w}x{h} {f}: two calls differ"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_planes_operator_is_the_composition_of_the_image_operator_and_the_encode(favlib, cuda, cases, size):
    """on the device, without the model: fav_color_transfer_yuv(...) == fav_rgb8_to_yuv(fav_color_transfer_rgb8(...))"""
    import torch
    c = cases[size]
    st, orig = torch.from_numpy(c["state"]).to(cuda), torch.from_numpy(c["orig"]).to(cuda)
    P = {m: favlib.color_transfer(st, orig, _cmatrix(favlib, m)) for m in MATRICES}
    for f in M.ALL_FORMATS:
        fused = favlib.color_transfer(st, orig, _cfmt(favlib, f))
        assert torch.equal(fused, favlib.rgb_to_yuv(P[f.matrix], _cfmt(favlib, f))), f"{size} {f}"


def test_operators_take_buffers_at_any_offset(favlib, cuda, cases):
    """no alignment is required: the byte buffers start 1 and 3 bytes into an allocation (the planes 1 and 3 floats), and the
    pattern in front of and behind every output survives"""
    import torch
    w, h = 131, 67
    c = cases[(w, h)]
    for off in (1, 3):
        stb = torch.zeros(3 * h * w + 8, dtype=torch.float32, device=cuda)
        stb[off:off + 3 * h * w] = torch.from_numpy(c["state"]).to(cuda).reshape(-1)
        st = stb[off:off + 3 * h * w].view(3, h, w)
        ob = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device=cuda)
        ob[off:off + h * w * 3] = torch.from_numpy(c["orig"]).to(cuda).reshape(-1)
        orig = ob[off:off + h * w * 3].view(h, w, 3)
        dst = _guarded(torch, cuda, h * w * 3 + 8)
        favlib.color_transfer(st, orig, favlib.YUV_BT709, out=dst[off:])
        _check_written(dst[off:], h * w * 3, c["P"]["709"], f"fav_color_transfer_rgb8 at offset {off}")
        assert (dst[:off] == PATTERN).all()
        for f in (M.Format("420", "center", "601", False), M.Format("420", "left", "709", False), M.Format("444", "center", "709", True)):
            n = M.frame_bytes(w, h, f)
            dst = _guarded(torch, cuda, n + 8)
            favlib.color_transfer(st, orig, _cfmt(favlib, f), out=dst[off:])
            _check_written(dst[off:], n, c["planes"][f], f"fav_color_transfer_yuv {f} at offset {off}")
            assert (dst[:off] == PATTERN).all()


def test_bad_arguments_are_einval_and_write_nothing(favlib, cuda):
    import torch
    st = torch.zeros((3, 4, 4), dtype=torch.float32, device=cuda)
    orig = torch.zeros((4, 4, 3), dtype=torch.uint8, device=cuda)
    out = _guarded(torch, cuda, 48)
    with pytest.raises(favlib.FavError) as e:
        favlib.color_transfer(st, orig, 2, out=out)
    assert "error -1" in str(e.value) and "matrix" in str(e.value)
    import ctypes as C
    L = favlib.lib()
    fmt = favlib.yuv_format()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.fav_color_transfer_rgb8(p(st), None, 4, 4, 0, p(out), None) == -1
    assert L.fav_color_transfer_rgb8(p(st), p(orig), 0, 4, 0, p(out), None) == -1
    assert L.fav_color_transfer_yuv(p(st), p(orig), 4, 4, None, p(out), None) == -1
    assert L.fav_color_transfer_yuv(None, p(orig), 4, 4, C.byref(fmt), p(out), None) == -1
    assert L.fav_color_transfer_yuv(p(st), p(orig), 1 << 15, 1 << 14, C.byref(fmt), p(out), None) == -1      # 2^29 pixels
    torch.cuda.synchronize()
    assert (out == PATTERN).all(), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ the stream forms
def _png_bytes_to_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_stream_forms_equal_the_model_and_leave_the_state_alone(favlib, cuda, golden_dir):
    import torch
    h, w = 48, 64
    net = favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)
    st = favlib.Stream(net, h, w)
    assert (st.Ho, st.Wo) == (h, w)
    f0, f1 = synth.smooth_frame(h, w, 1), synth.smooth_frame(h, w, 2)
    bw = synth.backward_flow(h, w, 3); fw = synth.forward_flow_from_backward(bw, 4)
    d0, d1 = torch.from_numpy(f0).to(cuda), torch.from_numpy(f1).to(cuda)
    png, nbytes = st.png_buffers()
    for step, (frame, dframe) in enumerate(((f0, d0), (f1, d1))):
        if step == 0:
            st.first_frame(dframe)
        else:
            st.next_frame_flow(dframe, torch.from_numpy(bw).to(cuda), torch.from_numpy(fw).to(cuda))
        before = st.state()
        state = before.cpu().numpy()
        for m in MATRICES:
            nbytes.zero_()
            st.encode_png_colors_into(dframe, _cmatrix(favlib, m), png, nbytes)
            torch.cuda.synchronize()
            got = _png_bytes_to_rgb(png[:int(nbytes.item())].cpu().numpy().tobytes())
            assert np.array_equal(got, CM.transfer(state, frame, m)), f"fav_stream_encode_png_colors, frame {step + 1}, BT.{m}"
        for f in (M.Format("420", "center", "601", False), M.Format("420", "left", "709", True), M.Format("444", "center", "709", False)):
            n = M.frame_bytes(w, h, f)
            buf = _guarded(torch, cuda, n)
            st.encode_yuv_colors_into(dframe, buf, _cfmt(favlib, f), capacity=n)
            _check_written(buf, n, M.rgb_to_yuv(CM.transfer(state, frame, f.matrix), f), f"fav_stream_encode_yuv_colors, frame {step + 1}, {f}")
            with pytest.raises(favlib.FavError) as e:
                st.encode_yuv_colors_into(dframe, buf, _cfmt(favlib, f), capacity=n - 1)
            assert "error -1" in str(e.value) and "buffer holds" in str(e.value)
        assert torch.equal(before, st.state()), f"frame {step + 1}: the state changed"
    # the guard of this test: the colours ARE another picture than the stylised frame
    assert not np.array_equal(CM.transfer(state, f1, "601"), M.quantise_f32_image(state))
    st.close(); net.close()


def test_stream_forms_refuse_a_stylised_size_that_is_not_the_frames(favlib, cuda, golden_dir):
    import torch
    h, w = 50, 70                                              # stylised frames are 52 x 72
    net = favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)
    st = favlib.Stream(net, h, w)
    assert (st.Ho, st.Wo) != (h, w)
    frame = torch.from_numpy(synth.smooth_frame(h, w, 5)).to(cuda)
    st.first_frame(frame)
    before = st.state()
    png, nbytes = st.png_buffers()
    png.fill_(PATTERN); nbytes.fill_(0x5A5A5A5A)
    f = M.Format("420", "center", "601", False)
    planes = _guarded(torch, cuda, M.frame_bytes(st.Wo, st.Ho, f))
    sizes = (f"{st.Wo}x{st.Ho}", f"{w}x{h}")
    with pytest.raises(favlib.FavError) as e:
        st.encode_png_colors_into(frame, favlib.YUV_BT601, png, nbytes)
    assert "error -4" in str(e.value) and all(s in str(e.value) for s in sizes), str(e.value)
    with pytest.raises(favlib.FavError) as e:
        st.encode_yuv_colors_into(frame, planes, _cfmt(favlib, f))
    assert "error -4" in str(e.value) and all(s in str(e.value) for s in sizes), str(e.value)
    torch.cuda.synchronize()
    assert (png == PATTERN).all() and int(nbytes.item()) == 0x5A5A5A5A and (planes == PATTERN).all(), "a refused call wrote"
    assert torch.equal(before, st.state())
    st.close(); net.close()


# ------------------------------------------------------------------------------------------------ the CLI
H_, W_, N_ = 48, 64, 4


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _run(args, **kw):
    return subprocess.run([STYLIZE] + args, capture_output=True, timeout=300, **kw)


@pytest.fixture(scope="module")
def first_clip(tmp_path_factory, golden_dir):
    """four 64 x 48 frames as PPM files, and the run WITHOUT the flag: the stylised frames the model is applied to"""
    d = tmp_path_factory.mktemp("colors")
    frames = [synth.smooth_frame(H_, W_, 80 + i) for i in range(N_)]
    for i, fr in enumerate(frames):
        S.write_ppm(str(d / f"frame_{i + 1:05d}.ppm"), fr)
    common = ["-input_pattern", str(d / "frame_%05d.ppm"), "-model_vid", os.path.join(golden_dir, "tiny_model.t7"), "-model_img", "self",
              "-estimate_flow", "1", "-poll_settle", "0"]
    plain = _run(["-output_prefix", str(d / "plain" / "out")] + common)
    assert plain.returncode == 0, plain.stderr.decode()
    stylised = [_png(d / "plain" / f"out-{i + 1:05d}.png") for i in range(N_)]
    return d, frames, common, stylised


def test_cli_three_sinks_agree_and_equal_the_model(favlib, first_clip):
    d, frames, common, stylised = first_clip
    flag = ["-original_colors", "1"]
    gpu = _run(["-output_prefix", str(d / "gpu" / "out"), "-png_encoder", "gpu"] + flag + common)
    host = _run(["-output_prefix", str(d / "host" / "out"), "-png_encoder", "host"] + flag + common)
    y4m = _run(["-output_y4m", str(d / "y4m" / "out.y4m")] + flag + common)
    for r in (gpu, host, y4m):
        assert r.returncode == 0, r.stderr.decode()
    f = M.Format("420", "center", "601", False)                # the default output format of a 48-row clip: BT.601, as for the PNGs
    header, planes = M.parse_y4m(open(d / "y4m" / "out.y4m", "rb").read(), lambda w, h: M.frame_bytes(w, h, f))
    assert header == f"YUV4MPEG2 W{W_} H{H_} F25:1 Ip A1:1 C420jpeg" and len(planes) == N_
    for i in range(N_):
        want = CM.transfer_bytes(stylised[i], frames[i], "601")
        a, b = _png(d / "gpu" / f"out-{i + 1:05d}.png"), _png(d / "host" / f"out-{i + 1:05d}.png")
        assert np.array_equal(a, want), f"frame {i + 1}, -png_encoder gpu: {int((a != want).sum())} bytes differ from the model"
        assert np.array_equal(b, a), f"frame {i + 1}: -png_encoder host differs from -png_encoder gpu"
        assert np.array_equal(planes[i], M.rgb_to_yuv(a, f)), f"frame {i + 1}: the planes are not the conversion of the PNG"
        assert not np.array_equal(want, stylised[i])             # the guard: the flag changes the picture


def test_cli_without_the_flag_nothing_changes(favlib, first_clip):
    """-original_colors 0 is the run without the option, file for file; with the flag -png_overlap 1 is the synchronous encode"""
    d, frames, common, stylised = first_clip
    off = _run(["-output_prefix", str(d / "off" / "out"), "-original_colors", "0"] + common)
    assert off.returncode == 0, off.stderr.decode()
    assert sorted(os.listdir(d / "off")) == sorted(os.listdir(d / "plain")) == [f"out-{i + 1:05d}.png" for i in range(N_)]
    for i in range(N_):
        assert open(d / "off" / f"out-{i + 1:05d}.png", "rb").read() == open(d / "plain" / f"out-{i + 1:05d}.png", "rb").read(), f"frame {i + 1}"
    ov = _run(["-output_prefix", str(d / "ov" / "out"), "-original_colors", "1", "-png_overlap", "1", "-y4m_matrix", "bt709"] + common)
    assert ov.returncode == 0, ov.stderr.decode()
    for i in range(N_):                                          # ... and -y4m_matrix chooses the luminance's matrix for PNGs as well
        assert np.array_equal(_png(d / "ov" / f"out-{i + 1:05d}.png"), CM.transfer_bytes(stylised[i], frames[i], "709")), f"frame {i + 1}"


def test_cli_y4m_input_estimated_flow_and_a_scene_cut(favlib, golden_dir, tmp_path):
    """the flag next to -input_y4m -estimate_flow 1 -scene_cut 0.5 on the six-frame clip with one cut: the original is the frame
    fav_yuv_to_rgb8 left on the device, and the recurrence (the cut included) is that of the run without the flag"""
    frames = S.cut_clip()
    f = M.Format("444", "center", "601", False)
    planes = [M.rgb_to_yuv(fr, f) for fr in frames]
    M.write_y4m(str(tmp_path / "clip.y4m"), M.y4m_header(S.CLIP_W, S.CLIP_H, f), planes)
    common = ["-input_y4m", str(tmp_path / "clip.y4m"), "-model_vid", os.path.join(golden_dir, "tiny_model.t7"), "-model_img", "self",
              "-estimate_flow", "1", "-scene_cut", "0.5", "-poll_settle", "0"]
    plain = _run(["-output_prefix", str(tmp_path / "plain" / "out"), "-scene_cut_log", str(tmp_path / "plain.log")] + common)
    col = _run(["-output_prefix", str(tmp_path / "col" / "out"), "-scene_cut_log", str(tmp_path / "col.log"), "-original_colors", "1"] + common)
    for r in (plain, col):
        assert r.returncode == 0, r.stderr.decode()
    assert open(tmp_path / "plain.log").read() == open(tmp_path / "col.log").read()
    assert [ln.split()[3] for ln in open(tmp_path / "col.log").read().splitlines()] == ["0", "0", "0", "1", "0", "0"]
    for i in range(6):
        orig = M.yuv_to_rgb(planes[i], S.CLIP_W, S.CLIP_H, f)
        want = CM.transfer_bytes(_png(tmp_path / "plain" / f"out-{i + 1:05d}.png"), orig, "601")
        got = _png(tmp_path / "col" / f"out-{i + 1:05d}.png")
        assert np.array_equal(got, want), f"frame {i + 1}: {int((got != want).sum())} bytes differ from the model"
