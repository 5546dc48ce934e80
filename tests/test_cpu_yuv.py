"""Host side of the Y4M route (no GPU needed): the numpy model of the YCbCr conversions (tests/util/yuv_model.py) against its own fp64
form and against Pillow, its chroma siting and odd sizes, libfav's YUV4MPEG2 header parser / formatter, and the combinations of
-input_y4m / -output_y4m that fav_stylize refuses before it opens a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import yuv_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
MATRIX_RANGE = [(m, r) for m in ("601", "709") for r in (False, True)]


def _lattice():
    """every combination of {0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 240, 254, 255} in the three channels"""
    v = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 240, 254, 255], np.uint8)
    g = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    return g.reshape(-1, 14, 3)                      # an image [196][14][3]


@pytest.fixture(scope="module")
def samples():
    """random bytes plus the lattice (0 and 255 in every channel), as two images; nothing is excluded"""
    rng = np.random.default_rng(20)
    return [rng.integers(0, 256, (512, 512, 3), dtype=np.uint8), _lattice()]


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


# ------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("matrix,full", MATRIX_RANGE)
def test_fp32_model_within_one_lsb_of_fp64_both_directions(samples, matrix, full):
    f = M.Format("444", "center", matrix, full)
    for img in samples:
        h, w = img.shape[:2]
        y32, y64 = M.rgb_to_yuv(img, f, np.float32), M.rgb_to_yuv(img, f, np.float64)
        assert _lsb(y32, y64) <= 1
        # the other direction on the same bytes read as (Y, Cb, Cr) planes: every triple, legal or not
        planes = np.concatenate([img[..., c].reshape(-1) for c in range(3)])
        assert _lsb(M.yuv_to_rgb(planes, w, h, f, np.float32), M.yuv_to_rgb(planes, w, h, f, np.float64)) <= 1


@pytest.mark.parametrize("matrix,full", MATRIX_RANGE)
def test_444_round_trip(samples, matrix, full):
    f = M.Format("444", "center", matrix, full)
    for img in samples:
        h, w = img.shape[:2]
        assert _lsb(M.yuv_to_rgb(M.rgb_to_yuv(img, f), w, h, f), img) <= (1 if full else 2)


def test_bt601_full_range_against_pillow(samples):
    Image = pytest.importorskip("PIL.Image")
    f = M.Format("444", "center", "601", True)
    for img in samples:
        h, w = img.shape[:2]
        pil = np.asarray(Image.fromarray(img).convert("YCbCr"))
        mine = np.stack(M.split_planes(M.rgb_to_yuv(img, f), w, h, f), -1)
        assert _lsb(mine, pil) <= 1
        pil_inv = np.asarray(Image.fromarray(img, "YCbCr").convert("RGB"))
        planes = np.concatenate([img[..., c].reshape(-1) for c in range(3)])
        assert _lsb(M.yuv_to_rgb(planes, w, h, f), pil_inv) <= 1


def test_constants_are_rounded_once_from_double():
    k = M.constants(M.Format("420", "center", "709", False))
    assert all(v.dtype == np.float32 for v in k.values())
    assert k["kg"] == np.float32(1.0 - 0.2126 - 0.0722) and k["sy"] == np.float32(219.0 / 255.0) and k["oy"] == 16
    assert k["kR"] == np.float32(2.0 * (1.0 - 0.2126) / (224.0 / 255.0))
    k = M.constants(M.Format("444", "center", "601", True), np.float64)
    assert k["sy"] == 1.0 and k["oy"] == 0.0 and k["cbs"] == 1.0 / (2.0 * (1.0 - 0.114))


# ------------------------------------------------------------------------------------------------ 2. siting and odd sizes
@pytest.mark.parametrize("siting,want", [("center", lambda x: 2 * x - 1), ("left", lambda x: 2 * x)])
def test_siting_of_the_decoded_chroma(siting, want):
    C = np.broadcast_to((4 * np.arange(20)).astype(np.uint8), (6, 20))            # C[j] = 4 j, constant along y
    for dt in (np.float32, np.float64):
        up = M.upsample_chroma(C, 40, 12, siting, dt)
        assert up.shape == (12, 40) and up.dtype == dt
        x = np.arange(1, 39)                                                      # the interior: the ends are clamped
        assert np.array_equal(up[:, 1:39], np.broadcast_to(want(x).astype(dt), (12, 38)))


@pytest.mark.parametrize("siting", ["center", "left"])
@pytest.mark.parametrize("size", [(16, 12), (5, 3), (1, 1)])
def test_constant_chroma_survives_420_exactly(siting, size):
    w, h = size
    for m, r in MATRIX_RANGE:
        f = M.Format("420", siting, m, r)
        img = np.empty((h, w, 3), np.uint8)
        img[...] = (200, 40, 90)                     # one colour: constant Cb, Cr, and luma as well
        yuv = M.rgb_to_yuv(img, f)
        _, cb, cr = M.split_planes(yuv, w, h, f)
        f444 = f._replace(chroma="444")
        _, cb4, cr4 = M.split_planes(M.rgb_to_yuv(img, f444), w, h, f444)
        assert (cb == cb4[0, 0]).all() and (cr == cr4[0, 0]).all()
        assert (M.upsample_chroma(cb, w, h, siting) == np.float32(cb4[0, 0])).all()
        assert (M.upsample_chroma(cr, w, h, siting) == np.float32(cr4[0, 0])).all()


@pytest.mark.parametrize("size", [(5, 3), (1, 1)])
def test_odd_sizes_have_ceil_planes(size):
    w, h = size
    rng = np.random.default_rng(w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for f in M.ALL_FORMATS:
        yuv = M.rgb_to_yuv(img, f)
        y, cb, cr = M.split_planes(yuv, w, h, f)
        want = (h, w) if f.chroma == "444" else ((h + 1) // 2, (w + 1) // 2)
        assert y.shape == (h, w) and cb.shape == want and cr.shape == want and yuv.size == M.frame_bytes(w, h, f)
        assert M.yuv_to_rgb(yuv, w, h, f).shape == (h, w, 3)
    # the missing partner is the replicated edge sample: the 5x3 planes equal those of the image padded to 6x4
    if size == (5, 3):
        pad = np.pad(img, ((0, 1), (0, 1), (0, 0)), mode="edge")
        f = M.Format("420", "center", "601", False)
        assert np.array_equal(M.split_planes(M.rgb_to_yuv(img, f), 5, 3, f)[1], M.split_planes(M.rgb_to_yuv(pad, f), 6, 4, f)[1])


def test_f32_input_is_quantised_like_image_save():
    x = np.array([-0.5, 0.0, 0.25, 100 / 255, 0.999, 1.0, 7.0], np.float32)
    img = np.broadcast_to(x, (3, 2, 7)).copy()
    q = M.quantise_f32_image(img)
    assert q.shape == (2, 7, 3) and q[0, :, 0].tolist() == [0, 0, 63, int(np.float32(100 / 255) * np.float32(255)), 254, 255, 255]
    f = M.Format()
    assert np.array_equal(M.rgb_f32_to_yuv(img, f), M.rgb_to_yuv(q, f))


# ------------------------------------------------------------------------------------------------ 3. YUV4MPEG2 headers
def test_header_tags_in_any_order_and_x_tags_verbatim(favlib):
    h = favlib.y4m_parse_header(b"YUV4MPEG2 XYSCSS=420MPEG2 A128:117 C420mpeg2 H1080 Ip F30000:1001 XCOLORRANGE=FULL W1920 XFOO=a:b\n")
    assert (h.W, h.H, h.fps_num, h.fps_den, h.aspect_num, h.aspect_den, chr(h.interlace)) == (1920, 1080, 30000, 1001, 128, 117, "p")
    assert (h.fmt.chroma, h.fmt.siting, h.fmt.matrix, h.fmt.full_range) == (favlib.YUV_420, favlib.YUV_SITING_LEFT, favlib.YUV_BT709, 1)
    assert h.xtags == b"XYSCSS=420MPEG2 XCOLORRANGE=FULL XFOO=a:b"
    out = favlib.y4m_format_header(h)
    assert out == b"YUV4MPEG2 W1920 H1080 F30000:1001 Ip A128:117 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=FULL XFOO=a:b\n"
    # the newline is optional for the parser, and bytes behind it are not its business
    assert favlib.y4m_parse_header(b"YUV4MPEG2 W4 H2").W == 4
    assert favlib.y4m_parse_header(b"YUV4MPEG2 W4 H2 C444\nFRAME\n" + bytes(24)).fmt.chroma == favlib.YUV_444


def test_header_defaults(favlib):
    h = favlib.y4m_parse_header(b"YUV4MPEG2 W640 H480\n")
    assert (h.fmt.chroma, h.fmt.siting, h.fmt.full_range, h.fmt.matrix) == (favlib.YUV_420, favlib.YUV_SITING_CENTER, 0, favlib.YUV_BT601)
    assert h.fps_den == 0 and h.aspect_num == -1 and h.interlace == 0 and h.xtags == b""
    assert favlib.y4m_format_header(h) == b"YUV4MPEG2 W640 H480 C420jpeg\n"
    for tag in (b"C420", b"C420jpeg"):
        f = favlib.y4m_parse_header(b"YUV4MPEG2 W8 H8 " + tag).fmt
        assert (f.chroma, f.siting) == (favlib.YUV_420, favlib.YUV_SITING_CENTER)
    assert favlib.y4m_parse_header(b"YUV4MPEG2 W1280 H719").fmt.matrix == favlib.YUV_BT601          # the matrix follows H
    assert favlib.y4m_parse_header(b"YUV4MPEG2 W1280 H720").fmt.matrix == favlib.YUV_BT709
    assert favlib.y4m_parse_header(b"YUV4MPEG2 W8 H8 XCOLORRANGE=LIMITED").fmt.full_range == 0
    assert chr(favlib.y4m_parse_header(b"YUV4MPEG2 W8 H8 I?").interlace) == "?"


@pytest.mark.parametrize("tag", ["C422", "C420p10", "C420paldv", "Cmono", "C444alpha", "It", "Ib", "Im"])
def test_header_refusals_name_the_tag(favlib, tag):
    with pytest.raises(favlib.FavError) as e:
        favlib.y4m_parse_header(f"YUV4MPEG2 W64 H48 F25:1 {tag} A1:1\n".encode())
    assert tag in str(e.value) and "error -4" in str(e.value), str(e.value)           # -4: valid, but outside what is covered


def test_header_malformed(favlib):
    for line, what in ((b"YUV4MPEG2 H48 F25:1\n", "W tag is missing"), (b"YUV4MPEG2 W64\n", "H tag is missing"),
                       (b"YUV4MPEG W64 H48\n", "YUV4MPEG2"), (b"P6 64 48 255\n", "YUV4MPEG2"),
                       (b"YUV4MPEG2 W64 H48 " + b"X" * 1100 + b"\n", "longer than 1024"),
                       (b"YUV4MPEG2 W64 H48 " + b"XA=1 " * 300, "longer than 1024"),
                       (b"YUV4MPEG2 W6x4 H48\n", "W6x4"), (b"YUV4MPEG2 W64 H48 F25\n", "F25"), (b"YUV4MPEG2 W64 H48 Q1\n", "Q1"),
                       (b"YUV4MPEG2 W64 H48 XCOLORRANGE=WIDE\n", "XCOLORRANGE=WIDE"), (b"YUV4MPEG2 W0 H48\n", "W0")):
        with pytest.raises(favlib.FavError) as e:
            favlib.y4m_parse_header(line)
        assert what in str(e.value) and "error -1" in str(e.value), (line[:40], str(e.value))
    # 1023 bytes and the newline still fit
    ok = b"YUV4MPEG2 W64 H48 X" + b"a" * (1023 - 19)
    assert len(ok) == 1023 and favlib.y4m_parse_header(ok + b"\n").W == 64


def test_header_format_then_parse_is_the_identity(favlib):
    for w, h, chroma, siting, full, fps, asp, il, xt in (
            (64, 48, favlib.YUV_420, favlib.YUV_SITING_CENTER, 0, (25, 1), (1, 1), ord("p"), b""),
            (1281, 721, favlib.YUV_420, favlib.YUV_SITING_LEFT, 1, (30000, 1001), (0, 0), ord("?"), b"XCOLORRANGE=FULL XYSCSS=420MPEG2"),
            (5, 3, favlib.YUV_444, favlib.YUV_SITING_CENTER, 0, (0, 0), (-1, 0), 0, b"XA XCOLORRANGE=LIMITED"),
            (1920, 1080, favlib.YUV_444, favlib.YUV_SITING_CENTER, 1, (60, 1), (1, 1), 0, b"XCOLORRANGE=FULL")):
        hd = favlib.Y4mHeader(w, h, fps[0], fps[1], asp[0], asp[1], il,
                              favlib.yuv_format(chroma, siting, favlib.YUV_BT709 if h >= 720 else favlib.YUV_BT601, full), xt)
        line = favlib.y4m_format_header(hd)
        assert line.startswith(b"YUV4MPEG2 W%d H%d" % (w, h)) and line.endswith(b"\n") and line.count(b"\n") == 1
        back = favlib.y4m_parse_header(line)
        for name, _ in favlib.Y4mHeader._fields_:
            a, b = getattr(hd, name), getattr(back, name)
            if name == "fmt":
                a, b = (a.chroma, a.siting, a.matrix, a.full_range), (b.chroma, b.siting, b.matrix, b.full_range)
            assert a == b, (name, a, b, line)
        assert favlib.y4m_format_header(back) == line
    # the range is written from the format: in place of a tag that disagrees, appended (FULL only) where there is none
    hd = favlib.y4m_parse_header(b"YUV4MPEG2 W8 H8 XA=1 XCOLORRANGE=FULL XB=2")
    hd.fmt.full_range = 0
    assert favlib.y4m_format_header(hd) == b"YUV4MPEG2 W8 H8 C420jpeg XA=1 XCOLORRANGE=LIMITED XB=2\n"
    hd = favlib.y4m_parse_header(b"YUV4MPEG2 W8 H8 XA=1")
    hd.fmt.full_range = 1
    assert favlib.y4m_format_header(hd) == b"YUV4MPEG2 W8 H8 C420jpeg XA=1 XCOLORRANGE=FULL\n"


def test_frame_bytes_and_format_checks_need_no_device(favlib):
    for f in M.ALL_FORMATS:
        cf = favlib.yuv_format(favlib.YUV_444 if f.chroma == "444" else favlib.YUV_420,
                               favlib.YUV_SITING_LEFT if f.siting == "left" else favlib.YUV_SITING_CENTER,
                               favlib.YUV_BT709 if f.matrix == "709" else favlib.YUV_BT601, f.full_range)
        for w, h in ((1, 1), (5, 3), (64, 48), (1280, 720), (1279, 719)):
            assert favlib.yuv_frame_bytes(w, h, cf) == M.frame_bytes(w, h, f)
    for w, h, cf, msg in ((0, 4, favlib.yuv_format(), "bad frame size"), (4, -1, favlib.yuv_format(), "bad frame size"),
                          (4, 4, favlib.yuv_format(chroma=2), "chroma must be"), (4, 4, favlib.yuv_format(siting=3), "siting must be"),
                          (4, 4, favlib.yuv_format(matrix=7), "matrix must be")):
        with pytest.raises(favlib.FavError) as e:
            favlib.yuv_frame_bytes(w, h, cf)
        assert msg in str(e.value)
    assert favlib.yuv_frame_bytes(4, 4, favlib.yuv_format(chroma=favlib.YUV_444, siting=3)) == 48        # the siting of 4:4:4 is not read
    for name in ("fav_yuv_frame_bytes", "fav_yuv_to_rgb8", "fav_rgb8_to_yuv", "fav_rgb_f32_to_yuv", "fav_stream_encode_yuv",
                 "fav_y4m_parse_header_host", "fav_y4m_format_header_host"):
        assert name in favlib.EXPORTS and hasattr(favlib.lib(), name)


# ------------------------------------------------------------------------------------------------ 4. fav_stylize: refused before a device is opened
@pytest.mark.parametrize("args,msg", [
    (["-input_y4m", "x.y4m", "-input_pattern", "f_%05d.ppm"], "INSTEAD of -input_pattern"),
    (["-backward", "-input_y4m", "x"], "-backward cannot be combined with -input_y4m"),
    (["-continue_with", "2", "-output_y4m", "x", "-input_pattern", "f_%05d.ppm"], "-continue_with 2 cannot be combined"),
    (["-continue_with", "3", "-input_y4m", "x"], "-continue_with 3 cannot be combined"),
    (["-streams", "a,b", "-input_y4m", "-"], "more than one -streams entry"),
    (["-streams", "a,b", "-input_pattern", "%S/f_%05d.ppm", "-output_y4m", "-"], "more than one -streams entry"),
    (["-input_y4m", "x", "-y4m_matrix", "bt2020"], "-y4m_matrix must be"),
    (["-input_y4m", "x", "-y4m_range", "tv"], "-y4m_range must be"),
    (["-input_y4m", "x", "-y4m_format", "422"], "-y4m_format must be"),
])
def test_fav_stylize_refuses_before_the_device(favlib, args, msg):
    r = subprocess.run([STYLIZE] + args + ["-estimate_flow", "1"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert r.returncode != 0 and msg in r.stderr, r.stderr
    assert "HIP" not in r.stderr and r.stdout == ""


def test_fav_stylize_dry_run_substitutes_the_stream_name_in_y4m_paths(favlib):
    import json
    r = subprocess.run([STYLIZE, "-streams", "a,b", "-input_y4m", "in/%S.y4m", "-output_y4m", "out/%S.y4m", "-estimate_flow", "1", "-dry_run", "1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert [(s["input_y4m"], s["output_y4m"]) for s in rec["streams"]] == [("in/a.y4m", "out/a.y4m"), ("in/b.y4m", "out/b.y4m")]
    r = subprocess.run([STYLIZE, "-streams", "a,b", "-input_y4m", "in/%S.y4m", "-output_y4m", "out.y4m", "-estimate_flow", "1", "-dry_run", "1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "-output_y4m must contain %S" in r.stderr


def test_waiting_for_a_file_is_announced_on_stderr_when_stdout_carries_the_stream(favlib, tmp_path):
    """the loaders' `Waiting for file` line (utils.lua:76) must not land in the video: with -output_y4m - it goes to stderr like every
    other message.  -load_probe runs the frame loop's loader for frame 2 without a device; the certainty file appears late."""
    import threading
    w, h = 8, 6
    (tmp_path / "frame_00002.ppm").write_bytes(b"P6\n%d %d\n255\n" % (w, h) + bytes(w * h * 3))
    (tmp_path / "backward_2_1.flo").write_bytes(np.float32(202021.25).tobytes() + np.int32(w).tobytes() + np.int32(h).tobytes() + bytes(w * h * 8))
    cert = tmp_path / "reliable_2_1.pgm"
    args = [STYLIZE, "-input_pattern", str(tmp_path / "frame_%05d.ppm"), "-flow_pattern", str(tmp_path / "backward_[%d]_{%d}.flo"),
            "-occlusions_pattern", str(tmp_path / "reliable_[%d]_{%d}.pgm"), "-load_probe", "2", "-poll_settle", "0.05", "-poll_timeout", "60"]
    for extra, stream in ((["-output_y4m", "-"], "stderr"), ([], "stdout")):
        if cert.exists():
            cert.unlink()
        p = subprocess.Popen(args + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL, bufsize=0)
        pipe = p.stderr if stream == "stderr" else p.stdout
        seen = b""
        while b"Waiting for file" not in seen:
            chunk = os.read(pipe.fileno(), 65536)
            assert chunk, "the probe ended without waiting for the certainty file"
            seen += chunk
        cert.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + bytes([255]) * (w * h))
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0, err
        if stream == "stderr":
            assert out == b"" and b'"ok": true' in seen + err
        else:
            assert b'"ok": true' in seen + out
