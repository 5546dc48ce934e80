"""The Y4M route on the GPU: the YCbCr kernels byte-equal to the fp32 numpy model (tests/util/yuv_model.py) over odd sizes, tails and
all twelve formats, written completely and nowhere else; fav_stream_encode_yuv against the stream's own 8-bit frame; and fav_stylize
with -input_y4m / -output_y4m against its PPM -> PNG route, through files and through pipes, and on a stream cut inside a frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import yuv_model as M  # noqa: E402

from fav_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
SIZES = [(2, 2), (5, 3), (17, 9), (64, 48), (131, 67), (258, 6)]            # (W, H): odd edges, one block, a tail narrower than a
GUARD, PATTERN = 64, 0xA5                                                    # lane's 8 columns, more than one block per row


@pytest.fixture(scope="module", autouse=True)
def _no_stale_hip_error(cuda):
    """HIP keeps the last error of any earlier call of the process until somebody asks for it, and torch asks after its next kernel
    launch.  A fav_vr / fav_stream finalised after its network leaves `invalid device ordinal` there (the binding now orders those
    finalisers: fav_amd.Net.close); this module's first allocation must not be what reports another module's leftover.  Only that one
    error is taken, with a warning that names it; anything else is raised."""
    import warnings
    import torch
    try:
        torch.zeros(1, device=cuda)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "invalid device ordinal" not in str(e):
            raise
        warnings.warn("a module that ran before tests/test_gpu_yuv.py left a HIP error behind: " + str(e).splitlines()[0])


def _cfmt(favlib, f):
    return favlib.yuv_format(favlib.YUV_444 if f.chroma == "444" else favlib.YUV_420,
                             favlib.YUV_SITING_LEFT if f.siting == "left" else favlib.YUV_SITING_CENTER,
                             favlib.YUV_BT709 if f.matrix == "709" else favlib.YUV_BT601, f.full_range)


def _inputs(w, h):
    """random bytes with 0, 255 and limited-range excursions planted; fp32 with values below 0, above 1 and exactly on k/255"""
    rng = np.random.default_rng(1000 * w + h)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    flat = rgb.reshape(-1)
    flat[rng.integers(0, flat.size, max(2, flat.size // 8))] = rng.choice(np.array([0, 255, 1, 15, 16, 235, 236, 240, 254], np.uint8), max(2, flat.size // 8))
    flat[0], flat[-1] = 0, 255
    n = M.frame_bytes(w, h, M.Format("444"))
    planes = rng.integers(0, 256, n, dtype=np.uint8)                        # read as planes of either sampling (the 4:2:0 ones are a prefix)
    planes[rng.integers(0, n, max(2, n // 8))] = rng.choice(np.array([0, 255, 5, 15, 16, 235, 236, 240, 241, 250], np.uint8), max(2, n // 8))
    f32 = rng.uniform(-0.3, 1.3, (3, h, w)).astype(np.float32)
    on = rng.random((3, h, w)) < 0.3
    f32[on] = (rng.integers(0, 256, int(on.sum())).astype(np.float32) / np.float32(255))
    return rgb, planes, f32


@pytest.fixture(scope="module")
def cases():
    """inputs and the model's outputs for every size and format, computed once"""
    out = {}
    for w, h in SIZES:
        rgb, planes, f32 = _inputs(w, h)
        for f in M.ALL_FORMATS:
            n = M.frame_bytes(w, h, f)
            out[(w, h, f)] = dict(rgb=rgb, planes=planes[:n], f32=f32, enc8=M.rgb_to_yuv(rgb, f), encf=M.rgb_f32_to_yuv(f32, f),
                                  dec=M.yuv_to_rgb(planes[:n], w, h, f))
    return out


def _guarded(torch, cuda, n):
    return torch.full((n + GUARD,), PATTERN, dtype=torch.uint8, device=cuda)


def _check_written(buf, n, want, what):
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n], want.reshape(-1)), f"{what}: {int((got[:n] != want.reshape(-1)).sum())} of {n} bytes differ from the model"
    assert (got[n:] == PATTERN).all(), f"{what}: bytes behind the frame were written"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_operators_equal_the_fp32_model_byte_for_byte(favlib, cuda, cases, size):
    import torch
    w, h = size
    for f in M.ALL_FORMATS:
        c, cf = cases[(w, h, f)], _cfmt(favlib, f)
        n = M.frame_bytes(w, h, f)
        assert favlib.yuv_frame_bytes(w, h, cf) == n
        rgb, planes, f32 = (torch.from_numpy(c[k]).to(cuda) for k in ("rgb", "planes", "f32"))
        for src, want, what in ((rgb, c["enc8"], "fav_rgb8_to_yuv"), (f32, c["encf"], "fav_rgb_f32_to_yuv")):
            a, b = _guarded(torch, cuda, n), _guarded(torch, cuda, n)
            favlib.rgb_to_yuv(src, cf, out=a); favlib.rgb_to_yuv(src, cf, out=b)
            _check_written(a, n, want, f"{what} {w}x{h} {f}")
            assert torch.equal(a, b), f"{what} {w}x{h} {f}: two calls differ"
        a, b = _guarded(torch, cuda, h * w * 3), _guarded(torch, cuda, h * w * 3)
        favlib.yuv_to_rgb8(planes, w, h, cf, out=a); favlib.yuv_to_rgb8(planes, w, h, cf, out=b)
        _check_written(a, h * w * 3, c["dec"], f"fav_yuv_to_rgb8 {w}x{h} {f}")
        assert torch.equal(a, b), f"fav_yuv_to_rgb8 {w}x{h} {f}: two calls differ"


def test_operators_take_buffers_at_any_byte_offset(favlib, cuda, cases):
    """no alignment is required of the caller's buffers: the same bytes from views that start 1 and 3 bytes into an allocation"""
    import torch
    w, h = 131, 67
    for f in (M.Format("420", "center", "601", False), M.Format("444", "center", "709", True)):
        c, cf = cases[(w, h, f)], _cfmt(favlib, f)
        n = M.frame_bytes(w, h, f)
        for off in (1, 3):
            src = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device=cuda)
            src[off:off + h * w * 3] = torch.from_numpy(c["rgb"]).to(cuda).reshape(-1)
            dst = _guarded(torch, cuda, n + 8)
            favlib.rgb_to_yuv(src[off:off + h * w * 3].view(h, w, 3), cf, out=dst[off:])
            _check_written(dst[off:], n, c["enc8"], f"fav_rgb8_to_yuv at offset {off}")
            assert (dst[:off] == PATTERN).all()
            pl = torch.zeros(n + 8, dtype=torch.uint8, device=cuda)
            pl[off:off + n] = torch.from_numpy(c["planes"]).to(cuda)
            out = _guarded(torch, cuda, h * w * 3 + 8)
            favlib.yuv_to_rgb8(pl[off:off + n], w, h, cf, out=out[off:])
            _check_written(out[off:], h * w * 3, c["dec"], f"fav_yuv_to_rgb8 at offset {off}")
            assert (out[:off] == PATTERN).all()


def test_stream_encode_yuv_is_the_conversion_of_the_streams_own_bytes(favlib, cuda, golden_dir):
    import torch
    h, w = 48, 64
    net = favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)
    st = favlib.Stream(net, h, w)
    f0, f1 = synth.smooth_frame(h, w, 1), synth.smooth_frame(h, w, 2)
    bw = synth.backward_flow(h, w, 3); fw = synth.forward_flow_from_backward(bw, 4)
    st.first_frame(torch.from_numpy(f0).to(cuda))
    _, out8 = st.next_frame_flow(torch.from_numpy(f1).to(cuda), torch.from_numpy(bw).to(cuda), torch.from_numpy(fw).to(cuda), want_u8=True)
    rgb8 = out8.cpu().numpy()
    assert rgb8.shape == (st.Ho, st.Wo, 3)
    for f in (M.Format("420", "center", "601", False), M.Format("444", "center", "601", False)):
        cf = _cfmt(favlib, f)
        n = M.frame_bytes(st.Wo, st.Ho, f)
        buf = _guarded(torch, cuda, n)
        st.encode_yuv_into(buf, cf, capacity=n)
        _check_written(buf, n, M.rgb_to_yuv(rgb8, f), f"fav_stream_encode_yuv {f}")
        short = _guarded(torch, cuda, n)
        with pytest.raises(favlib.FavError) as e:
            st.encode_yuv_into(short, cf, capacity=n - 1)
        assert "error -1" in str(e.value) and "buffer holds" in str(e.value)
        torch.cuda.synchronize()
        assert (short == PATTERN).all(), "a refused call wrote"
    st.close(); net.close()


# ------------------------------------------------------------------------------------------------ the CLI
H_, W_, N_ = 48, 64, 4


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _clip(tmp, f, extra):
    """a 4-frame 64x48 clip as clip.y4m AND as the PPMs of the model's decode of that file: both routes see identical RGB"""
    frames = [M.rgb_to_yuv(synth.smooth_frame(H_, W_, 60 + i), f) for i in range(N_)]
    M.write_y4m(str(tmp / "clip.y4m"), M.y4m_header(W_, H_, f, extra), frames)
    for i, fr in enumerate(frames):
        with open(tmp / f"frame_{i + 1:05d}.ppm", "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W_, H_) + M.yuv_to_rgb(fr, W_, H_, f).tobytes())
    return frames


def _run(args, **kw):
    return subprocess.run([STYLIZE] + args, capture_output=True, timeout=300, **kw)


@pytest.mark.parametrize("f,extra,opts", [
    (M.Format("420", "center", "601", False), "F30000:1001 Ip A1:1 XYSCSS=420JPEG XFAV=test", []),
    (M.Format("444", "center", "601", True), "F25:1 A4:3", ["-y4m_matrix", "bt601"]),
], ids=["420jpeg-limited", "444-full-bt601"])
def test_cli_y4m_route_equals_ppm_png_route(favlib, golden_dir, tmp_path, f, extra, opts):
    _clip(tmp_path, f, extra)
    common = ["-model_vid", os.path.join(golden_dir, "tiny_model.t7"), "-model_img", "self", "-estimate_flow", "1", "-poll_settle", "0"]
    a = _run(["-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-output_prefix", str(tmp_path / "a" / "out")] + common)
    assert a.returncode == 0, a.stderr.decode()
    (tmp_path / "b").mkdir()
    b = _run(["-input_y4m", str(tmp_path / "clip.y4m"), "-output_y4m", str(tmp_path / "b" / "out.y4m"), "-output_prefix", str(tmp_path / "b" / "out")]
             + common + opts)
    assert b.returncode == 0, b.stderr.decode()
    assert b"Writing output image" in b.stdout                                  # a file: the messages stay on stdout
    data = open(tmp_path / "b" / "out.y4m", "rb").read()
    header, frames = M.parse_y4m(data, lambda w, h: M.frame_bytes(w, h, f))
    want_tags = ["YUV4MPEG2", f"W{W_}", f"H{H_}"] + [t for t in extra.split() if t[0] in "FIA"] + [M.C_TAG[(f.chroma, f.siting)]] + \
                [t for t in extra.split() if t[0] == "X"] + (["XCOLORRANGE=FULL"] if f.full_range else [])
    assert header.split(" ") == want_tags
    assert len(frames) == N_ and len(data) == len(header) + 1 + N_ * (6 + M.frame_bytes(W_, H_, f))
    for i, fr in enumerate(frames):
        want = M.rgb_to_yuv(_png(tmp_path / "a" / f"out-{i + 1:05d}.png"), f)
        assert np.array_equal(fr, want), f"frame {i + 1}: {int((fr != want).sum())} bytes differ from the PNG route's"
    assert [p for p in os.listdir(tmp_path / "b") if p.endswith(".png")] == [], "the Y4M route wrote PNG files"
    # the same through pipes: stdout is the stream and nothing else, the messages are on stderr
    with open(tmp_path / "clip.y4m", "rb") as fh:
        p = _run(["-input_y4m", "-", "-output_y4m", "-"] + common + opts + ["-timing", "1"], stdin=fh)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout[:9] == b"YUV4MPEG2" and p.stdout == data
    assert b"Writing output image" in p.stderr and b"fps_end_to_end" in p.stderr and b"Model loaded." in p.stderr


def test_cli_mixed_routes_and_num_frames(favlib, golden_dir, tmp_path):
    """the two options are independent: Y4M in with PNG out equals the PPM route's PNGs; PPM in with Y4M out (-y4m_format 420mpeg2,
    default header) equals their conversion; -num_frames ends the stream early"""
    f = M.Format("420", "center", "601", False)
    _clip(tmp_path, f, "F25:1 Ip A1:1")
    common = ["-model_vid", os.path.join(golden_dir, "tiny_model.t7"), "-model_img", "self", "-estimate_flow", "1", "-poll_settle", "0", "-num_frames", "3"]
    a = _run(["-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-output_prefix", str(tmp_path / "a" / "out")] + common)
    b = _run(["-input_y4m", str(tmp_path / "clip.y4m"), "-output_prefix", str(tmp_path / "b" / "out")] + common)
    c = _run(["-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-output_y4m", str(tmp_path / "c" / "out.y4m"), "-y4m_format", "420mpeg2"] + common)
    for r in (a, b, c):
        assert r.returncode == 0, r.stderr.decode()
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == [f"out-{i:05d}.png" for i in (1, 2, 3)]
    for i in (1, 2, 3):
        assert np.array_equal(_png(tmp_path / "a" / f"out-{i:05d}.png"), _png(tmp_path / "b" / f"out-{i:05d}.png"))
    fo = M.Format("420", "left", "601", False)
    header, frames = M.parse_y4m(open(tmp_path / "c" / "out.y4m", "rb").read(), lambda w, h: M.frame_bytes(w, h, fo))
    assert header == f"YUV4MPEG2 W{W_} H{H_} F25:1 Ip A1:1 C420mpeg2" and len(frames) == 3
    for i, fr in enumerate(frames):
        assert np.array_equal(fr, M.rgb_to_yuv(_png(tmp_path / "a" / f"out-{i + 1:05d}.png"), fo))


def test_cli_truncated_stream_is_an_error_after_the_complete_frames(favlib, golden_dir, tmp_path):
    """host-side input validation: the stream ends in the middle of frame 3"""
    f = M.Format("420", "center", "601", False)
    _clip(tmp_path, f, "F25:1 Ip A1:1")
    data = open(tmp_path / "clip.y4m", "rb").read()
    nb = M.frame_bytes(W_, H_, f)
    hdr = data.index(b"\n") + 1
    cut = hdr + 2 * (6 + nb) + 6 + nb // 2
    open(tmp_path / "cut.y4m", "wb").write(data[:cut])
    r = _run(["-input_y4m", str(tmp_path / "cut.y4m"), "-output_y4m", str(tmp_path / "out.y4m"), "-model_vid", os.path.join(golden_dir, "tiny_model.t7"),
              "-model_img", "self", "-estimate_flow", "1"])
    assert r.returncode != 0 and b"ends inside frame 3" in r.stderr, r.stderr.decode()
    out = open(tmp_path / "out.y4m", "rb").read()
    _, frames = M.parse_y4m(out, lambda w, h: nb)
    assert len(frames) == 2 and len(out) == out.index(b"\n") + 1 + 2 * (6 + nb)
    # ... and a stream that ends at a frame boundary is simply a shorter clip
    open(tmp_path / "two.y4m", "wb").write(data[:hdr + 2 * (6 + nb)])
    r = _run(["-input_y4m", str(tmp_path / "two.y4m"), "-output_y4m", str(tmp_path / "out2.y4m"), "-model_vid", os.path.join(golden_dir, "tiny_model.t7"),
              "-model_img", "self", "-estimate_flow", "1"])
    assert r.returncode == 0, r.stderr.decode()
    assert open(tmp_path / "out2.y4m", "rb").read() == out


def _write_flo(path, uv):
    h, w = uv.shape[:2]
    with open(path, "wb") as fh:
        fh.write(np.float32(202021.25).tobytes() + np.int32(w).tobytes() + np.int32(h).tobytes() + np.ascontiguousarray(uv, np.float32).tobytes())


def test_cli_stdout_is_the_stream_and_nothing_else_while_a_flow_file_is_awaited(favlib, golden_dir, tmp_path):
    """-output_y4m - next to -flow_pattern / -forward_flow_pattern whose producer is still at work: frame 3's forward flow appears only
    after the loader has announced that it waits for it.  The announcement belongs on stderr; stdout parses as exactly 4 frames and
    equals what the same run writes into a file."""
    f = M.Format("420", "center", "601", False)
    _clip(tmp_path, f, "F25:1 Ip A1:1")
    (tmp_path / "flow").mkdir()
    late = None
    for i in range(2, N_ + 1):
        bw = synth.backward_flow(H_, W_, 300 + i); fw = synth.forward_flow_from_backward(bw, 400 + i)
        _write_flo(tmp_path / "flow" / f"backward_{i}_{i - 1}.flo", bw)
        if i == 3:
            late = (tmp_path / "flow" / f"forward_{i - 1}_{i}.flo", fw)
        else:
            _write_flo(tmp_path / "flow" / f"forward_{i - 1}_{i}.flo", fw)
    args = [STYLIZE, "-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-flow_pattern", str(tmp_path / "flow" / "backward_[%d]_{%d}.flo"),
            "-forward_flow_pattern", str(tmp_path / "flow" / "forward_{%d}_[%d].flo"), "-model_vid", os.path.join(golden_dir, "tiny_model.t7"),
            "-model_img", "self", "-poll_settle", "0.05", "-poll_timeout", "120"]
    p = subprocess.Popen(args + ["-output_y4m", "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL, bufsize=0)
    err = b""
    while b"Waiting for file" not in err:                    # the loader has looked and not found it (or the program has ended: a failure)
        chunk = os.read(p.stderr.fileno(), 65536)
        assert chunk, "the program ended without waiting for the missing flow file: " + err.decode()
        err += chunk
    _write_flo(late[0], late[1])
    out, rest = p.communicate(timeout=300)
    err += rest
    assert p.returncode == 0, err.decode()
    assert str(late[0]).encode() in err and b"Writing output image" in err
    header, frames = M.parse_y4m(out, lambda w, h: M.frame_bytes(w, h, f))
    assert header == f"YUV4MPEG2 W{W_} H{H_} F25:1 Ip A1:1 C420jpeg" and len(frames) == N_
    assert len(out) == len(header) + 1 + N_ * (6 + M.frame_bytes(W_, H_, f))
    r = _run(args[1:] + ["-output_y4m", str(tmp_path / "out.y4m")])
    assert r.returncode == 0, r.stderr.decode()
    assert open(tmp_path / "out.y4m", "rb").read() == out
