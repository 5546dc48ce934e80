"""The 4:2:2 / 9- to 16-bit Y4M route on the GPU (include/fav_yuv.h): the kernels of csrc/kernels_yuv_layout.hip equal to the fp32 numpy
model (tests/util/yuv_layout_model.py) sample for sample over one-sample, full, partial and several blocks, written completely and
nowhere else, at any byte offset; depth 8 in 4:2:0 / 4:4:4 equal to today's operators; fav_stream_encode_yuv_layout against the model on
the stream's own state; and fav_stylize with deep streams in and out."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import yuv_model as M8  # noqa: E402
import yuv_layout_model as M  # noqa: E402

from fav_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
# (W, H): one sample, one chroma sample, partial in both, one full block, partial in x and y, two full blocks, partial in both next to
# full ones, several blocks per row and column
SIZES = [(1, 1), (2, 2), (5, 3), (8, 2), (9, 3), (16, 4), (17, 5), (64, 48)]
GUARD, PATTERN = 64, 0xA5
# every sampling x matrix x range at depths 8, 10, 16; depths 9, 12, 14 on one sampling each
LAYOUTS = [M.Layout(c, s, m, r, d) for (c, s), m, r, d in itertools.product(M.SAMPLINGS, ("601", "709"), (False, True), (8, 10, 16))] + \
          [M.Layout("420", "left", "709", False, 9), M.Layout("422", "left", "601", True, 12), M.Layout("444", "center", "601", False, 14)]


def _cl(favlib, lay):
    return favlib.yuv_layout({"420": favlib.YUV_420, "444": favlib.YUV_444, "422": favlib.YUV_422}[lay.chroma],
                             favlib.YUV_SITING_LEFT if lay.siting == "left" else favlib.YUV_SITING_CENTER,
                             favlib.YUV_BT709 if lay.matrix == "709" else favlib.YUV_BT601, lay.full_range, lay.depth)


def _inputs(w, h):
    """random bytes with the extremes planted; random samples over the whole 16-bit range (out-of-range values for every depth below
    16) and over the bytes; fp32 below 0, above 1, on k/255 and between grey levels"""
    rng = np.random.default_rng(1000 * w + h)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    flat = rgb.reshape(-1)
    k = max(2, flat.size // 8)
    flat[rng.integers(0, flat.size, k)] = rng.choice(np.array([0, 255, 1, 15, 16, 235, 236, 240, 254], np.uint8), k)
    flat[0], flat[-1] = 0, 255
    n = 3 * w * h                                                               # 4:4:4; the other samplings read a prefix
    s16 = rng.integers(0, 65536, n).astype(np.uint16)
    s16[rng.integers(0, n, max(2, n // 8))] = rng.choice(np.array([0, 65535, 64, 940, 960, 1023, 1024, 4095, 32768], np.uint16), max(2, n // 8))
    s8 = rng.integers(0, 256, n).astype(np.uint8)
    f32 = rng.uniform(-0.3, 1.3, (3, h, w)).astype(np.float32)
    on = rng.random((3, h, w)) < 0.3
    f32[on] = (rng.integers(0, 256, int(on.sum())).astype(np.float32) / np.float32(255))
    return rgb, s8, s16, f32


@pytest.fixture(scope="module")
def cases():
    """inputs and the model's outputs (as the frame's BYTES) for every size and layout, computed once and never changed"""
    out = {}
    for w, h in SIZES:
        rgb, s8, s16, f32 = _inputs(w, h)
        for lay in LAYOUTS:
            ns = M.frame_samples(w, h, lay)
            planes = (s8 if lay.depth == 8 else s16)[:ns]
            out[(w, h, lay)] = dict(rgb=rgb, f32=f32, planes=M.payload(planes, lay), enc8=M.payload(M.rgb_to_yuv(rgb, lay), lay),
                                    encf=M.payload(M.rgb_f32_to_yuv(f32, lay), lay), dec=M.yuv_to_rgb(planes, w, h, lay))
    for c in out.values():
        for v in c.values():
            v.setflags(write=False)
    return out


def _guarded(torch, cuda, n, off=0):
    """n bytes inside a guard pattern, starting `off` bytes behind a 64-byte boundary: (whole buffer, the view to write into)"""
    buf = torch.full((GUARD + off + n + GUARD,), PATTERN, dtype=torch.uint8, device=cuda)
    return buf, buf[GUARD + off:GUARD + off + n]


def _check_written(buf, view_off, n, want, what):
    got = buf.cpu().numpy()
    body = got[view_off:view_off + n]
    want = np.asarray(want).reshape(-1).view(np.uint8)
    assert np.array_equal(body, want), f"{what}: {int((body != want).sum())} of {n} bytes differ from the model"
    assert (got[:view_off] == PATTERN).all() and (got[view_off + n:] == PATTERN).all(), f"{what}: bytes outside the buffer were written"


def _three_operators(favlib, torch, cuda, c, lay, w, h, off=0):
    cl = _cl(favlib, lay)
    n = M.frame_bytes(w, h, lay)
    assert favlib.yuv_layout_frame_bytes(w, h, cl) == n == c["planes"].size
    what = f"{w}x{h} {lay} offset {off}"
    if off:       # the inputs too start `off` bytes into an allocation
        hold = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device=cuda)
        hold[off:off + h * w * 3] = torch.from_numpy(c["rgb"].copy()).to(cuda).reshape(-1)
        rgb = hold[off:off + h * w * 3].view(h, w, 3)
        holdp = torch.zeros(n + 8, dtype=torch.uint8, device=cuda)
        holdp[off:off + n] = torch.from_numpy(c["planes"].copy()).to(cuda)
        planes = holdp[off:off + n]
    else:
        rgb, planes = torch.from_numpy(c["rgb"].copy()).to(cuda), torch.from_numpy(c["planes"].copy()).to(cuda)
    f32 = torch.from_numpy(c["f32"].copy()).to(cuda)
    for src, want, name in ((rgb, c["enc8"], "fav_rgb8_to_yuv_layout"), (f32, c["encf"], "fav_rgb_f32_to_yuv_layout")):
        buf, view = _guarded(torch, cuda, n, off)
        favlib.rgb_to_yuv_layout(src, cl, out=view)
        _check_written(buf, GUARD + off, n, want, f"{name} {what}")
    buf, view = _guarded(torch, cuda, h * w * 3, off)
    favlib.yuv_layout_to_rgb8(planes, w, h, cl, out=view)
    _check_written(buf, GUARD + off, h * w * 3, c["dec"], f"fav_yuv_layout_to_rgb8 {what}")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_three_operators_equal_the_fp32_model_sample_for_sample(favlib, cuda, cases, size):
    import torch
    w, h = size
    for lay in LAYOUTS:
        _three_operators(favlib, torch, cuda, cases[(w, h, lay)], lay, w, h)


@pytest.mark.parametrize("off", [1, 3])
def test_buffers_at_odd_byte_offsets(favlib, cuda, cases, off):
    """no alignment is required: planes (two-byte samples at an odd address) and images that start 1 and 3 bytes into an allocation, on
    a size with full and partial blocks"""
    import torch
    w, h = 17, 5
    for lay in LAYOUTS:
        if (lay.matrix, lay.full_range) == ("709", False):
            _three_operators(favlib, torch, cuda, cases[(w, h, lay)], lay, w, h, off)


def test_depth_8_is_todays_bytes(favlib, cuda, cases):
    """4:2:0 (both sitings) and 4:4:4 at depth 8: the bytes of fav_yuv_to_rgb8 / fav_rgb8_to_yuv / fav_rgb_f32_to_yuv"""
    import torch
    for (w, h), lay in itertools.product([(5, 3), (17, 5), (64, 48)], [l for l in LAYOUTS if l.depth == 8 and l.chroma != "422"]):
        c, cl = cases[(w, h, lay)], _cl(favlib, lay)
        cf = favlib.yuv_format(cl.chroma, cl.siting, cl.matrix, lay.full_range)
        rgb, planes, f32 = (torch.from_numpy(c[k].copy()).to(cuda) for k in ("rgb", "planes", "f32"))
        assert torch.equal(favlib.rgb_to_yuv_layout(rgb, cl), favlib.rgb_to_yuv(rgb, cf)), (w, h, lay)
        assert torch.equal(favlib.rgb_to_yuv_layout(f32, cl), favlib.rgb_to_yuv(f32, cf)), (w, h, lay)
        assert torch.equal(favlib.yuv_layout_to_rgb8(planes, w, h, cl), favlib.yuv_to_rgb8(planes, w, h, cf)), (w, h, lay)


def test_bad_fields_are_refused_by_name_and_nothing_is_written(favlib, cuda):
    import torch
    rgb = torch.zeros((4, 8, 3), dtype=torch.uint8, device=cuda)
    out = torch.full((256,), PATTERN, dtype=torch.uint8, device=cuda)
    for cl, msg in ((favlib.yuv_layout(depth=11), "depth must be"), (favlib.yuv_layout(chroma=5), "chroma must be"),
                    (favlib.yuv_layout(struct_bytes=20), "struct_bytes must be")):
        with pytest.raises(favlib.FavError) as e:
            favlib._check(favlib.lib().fav_rgb8_to_yuv_layout(favlib._p(rgb), 8, 4, favlib.C.byref(cl), favlib._p(out), favlib._stream()))
        assert msg in str(e.value)
    torch.cuda.synchronize()
    assert (out == PATTERN).all()


def test_stream_encode_yuv_layout_is_the_model_on_the_streams_state(favlib, cuda, golden_dir):
    import torch
    h, w = 48, 64
    net = favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)
    st = favlib.Stream(net, h, w)
    f0, f1 = synth.smooth_frame(h, w, 1), synth.smooth_frame(h, w, 2)
    bw = synth.backward_flow(h, w, 3); fw = synth.forward_flow_from_backward(bw, 4)
    st.first_frame(torch.from_numpy(f0).to(cuda))
    st.next_frame_flow(torch.from_numpy(f1).to(cuda), torch.from_numpy(bw).to(cuda), torch.from_numpy(fw).to(cuda))
    before = st.state().cpu().numpy()
    # depth 10 and 16: the floats enter unquantised; depth 8 in 4:2:2: image.save's truncation in front
    for lay in (M.Layout("420", "center", "601", False, 10), M.Layout("422", "left", "709", True, 16), M.Layout("422", "left", "601", False, 8)):
        cl = _cl(favlib, lay)
        n = M.frame_bytes(st.Wo, st.Ho, lay)
        buf, view = _guarded(torch, cuda, n)
        st.encode_yuv_layout_into(view, cl, capacity=n)
        _check_written(buf, GUARD, n, M.payload(M.rgb_f32_to_yuv(before, lay), lay), f"fav_stream_encode_yuv_layout {lay}")
        buf, view = _guarded(torch, cuda, n)
        with pytest.raises(favlib.FavError) as e:
            st.encode_yuv_layout_into(view, cl, capacity=n - 1)
        assert "error -1" in str(e.value) and "buffer holds" in str(e.value)
        torch.cuda.synchronize()
        assert (buf == PATTERN).all(), "a refused call wrote"
    # the deep planes carry more than the 8-bit image: they are not the conversion of its bytes
    lay = M.Layout("444", "center", "601", True, 10)
    assert not np.array_equal(M.rgb_f32_to_yuv(before, lay), M.rgb_to_yuv(M8.quantise_f32_image(before), lay))
    assert np.array_equal(st.state().cpu().numpy().view(np.uint32), before.view(np.uint32)), "the state changed"
    st.close(); net.close()


# ------------------------------------------------------------------------------------------------ the CLI
H_, W_, N_ = 48, 64, 4
F8 = M8.Format("420", "center", "601", False)


def _clip8(tmp):
    frames = [M8.rgb_to_yuv(synth.smooth_frame(H_, W_, 60 + i), F8) for i in range(N_)]
    M8.write_y4m(str(tmp / "clip.y4m"), M8.y4m_header(W_, H_, F8, "F25:1 Ip A1:1 XFAV=test"), frames)
    return frames


def _run(args, **kw):
    return subprocess.run([STYLIZE] + args, capture_output=True, timeout=300, **kw)


def _common(golden_dir):
    return ["-model_vid", os.path.join(golden_dir, "tiny_model.t7"), "-model_img", "self", "-estimate_flow", "1", "-poll_settle", "0"]


def _write_deep(path, frames8, depth=10):
    """the 8-bit stream's samples x 2^(D-8) as a C420pD limited-range stream"""
    with open(path, "wb") as fh:
        fh.write(f"YUV4MPEG2 W{W_} H{H_} F25:1 Ip A1:1 C420p{depth} XFAV=test\n".encode())
        for fr in frames8:
            fh.write(b"FRAME\n" + (fr.astype("<u2") << (depth - 8)).tobytes())


def test_cli_deep_input_equals_the_8_bit_run(favlib, golden_dir, tmp_path):
    """(a) a C420p10 stream whose samples are the 8-bit stream's x 4 decodes to the same RGB bytes (limited range: a power of two
    commutes with every rounding), so with -y4m_pixel_format 420jpeg it gives the 8-bit run's stream, header included"""
    frames = _clip8(tmp_path)
    _write_deep(tmp_path / "deep.y4m", frames)
    a = _run(["-input_y4m", str(tmp_path / "clip.y4m"), "-output_y4m", str(tmp_path / "a.y4m")] + _common(golden_dir))
    assert a.returncode == 0, a.stderr.decode()
    b = _run(["-input_y4m", str(tmp_path / "deep.y4m"), "-output_y4m", str(tmp_path / "b.y4m"), "-y4m_pixel_format", "420jpeg"] + _common(golden_dir))
    assert b.returncode == 0, b.stderr.decode()
    da, db = open(tmp_path / "a.y4m", "rb").read(), open(tmp_path / "b.y4m", "rb").read()
    assert da[:da.index(b"\n")] == f"YUV4MPEG2 W{W_} H{H_} F25:1 Ip A1:1 C420jpeg XFAV=test".encode()
    assert len(da) == da.index(b"\n") + 1 + N_ * (6 + M8.frame_bytes(W_, H_, F8)) and db == da


def test_cli_deep_output_and_default_output(favlib, cuda, golden_dir, tmp_path):
    """(b) 8-bit in, -y4m_pixel_format 422p10: the header says C422p10 and every payload is what fav_stream_encode_yuv_layout gives for
    the same stream in process; (c) with no format option a deep input's tag is the output's"""
    import torch
    frames = _clip8(tmp_path)
    r = _run(["-input_y4m", str(tmp_path / "clip.y4m"), "-output_y4m", str(tmp_path / "out.y4m"), "-y4m_pixel_format", "422p10"] + _common(golden_dir))
    assert r.returncode == 0, r.stderr.decode()
    lay = M.Layout("422", "left", "601", False, 10)
    cl = _cl(favlib, lay)
    nb = favlib.yuv_layout_frame_bytes(W_, H_, cl)
    assert nb == M.frame_bytes(W_, H_, lay) == 2 * (W_ * H_ + 2 * H_ * (W_ // 2))
    data = open(tmp_path / "out.y4m", "rb").read()
    header, got = M8.parse_y4m(data, lambda w, h: nb)
    assert header == f"YUV4MPEG2 W{W_} H{H_} F25:1 Ip A1:1 C422p10 XFAV=test"
    assert len(got) == N_ and len(data) == len(header) + 1 + N_ * (6 + nb)
    # the same stream in process: the frames are the decode of the input's planes (the kernels equal the model: above)
    rgb = [torch.from_numpy(M8.yuv_to_rgb(fr, W_, H_, F8)).to(cuda) for fr in frames]
    net = favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)
    st = favlib.Stream(net, H_, W_)
    buf = torch.empty(nb, dtype=torch.uint8, device=cuda)
    for i in range(N_):
        if i == 0:
            st.first_frame(rgb[0])
        else:
            st.next_frame_estimate(rgb[i], rgb[i - 1], use_structure=True, batched=True)
        st.encode_yuv_layout_into(buf, cl)
        want = buf.cpu().numpy()
        assert np.array_equal(got[i], want), f"frame {i + 1}: {int((got[i] != want).sum())} bytes differ from the in-process encode"
    st.close(); net.close()
    # (c)
    _write_deep(tmp_path / "deep.y4m", frames, 12)
    r = _run(["-input_y4m", str(tmp_path / "deep.y4m"), "-output_y4m", str(tmp_path / "same.y4m"), "-num_frames", "2"] + _common(golden_dir))
    assert r.returncode == 0, r.stderr.decode()
    data = open(tmp_path / "same.y4m", "rb").read()
    n12 = M.frame_bytes(W_, H_, M.Layout("420", "center", "601", False, 12))
    assert data[:data.index(b"\n")] == f"YUV4MPEG2 W{W_} H{H_} F25:1 Ip A1:1 C420p12 XFAV=test".encode()
    assert len(data) == data.index(b"\n") + 1 + 2 * (6 + n12)


def test_cli_truncated_deep_stream_is_an_error_after_the_complete_frames(favlib, golden_dir, tmp_path):
    """(d) a C420p10 stream that ends in the middle of frame 3"""
    frames = _clip8(tmp_path)
    _write_deep(tmp_path / "deep.y4m", frames)
    data = open(tmp_path / "deep.y4m", "rb").read()
    nb = M.frame_bytes(W_, H_, M.Layout("420", "center", "601", False, 10))
    hdr = data.index(b"\n") + 1
    assert len(data) == hdr + N_ * (6 + nb)
    open(tmp_path / "cut.y4m", "wb").write(data[:hdr + 2 * (6 + nb) + 6 + nb // 2])
    r = _run(["-input_y4m", str(tmp_path / "cut.y4m"), "-output_y4m", str(tmp_path / "out.y4m")] + _common(golden_dir))
    assert r.returncode != 0 and b"ends inside frame 3" in r.stderr, r.stderr.decode()
    out = open(tmp_path / "out.y4m", "rb").read()
    _, got = M8.parse_y4m(out, lambda w, h: nb)
    assert len(got) == 2 and len(out) == out.index(b"\n") + 1 + 2 * (6 + nb)
