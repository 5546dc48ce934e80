"""Host side of the 4:2:2 / 9- to 16-bit Y4M route (include/fav_yuv.h; no GPU needed): the exports, libfav's stream-header parser and
formatter for every C tag, fav_yuv_layout_frame_bytes, the numpy model (tests/util/yuv_layout_model.py) against its own fp64 form and
round the RGB cube, the invariant the deep-input CLI test rests on, and what fav_stylize refuses before it opens a device."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import yuv_model as M8  # noqa: E402
import yuv_layout_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
DEEP = (9, 10, 12, 14, 16)


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(fav_[a-z0-9_]+)\s*\(", hdr))


def _clayout(favlib, lay, **kw):
    return favlib.yuv_layout({"420": favlib.YUV_420, "444": favlib.YUV_444, "422": favlib.YUV_422}[lay.chroma],
                             favlib.YUV_SITING_LEFT if lay.siting == "left" else favlib.YUV_SITING_CENTER,
                             favlib.YUV_BT709 if lay.matrix == "709" else favlib.YUV_BT601, lay.full_range, lay.depth, **kw)


# ------------------------------------------------------------------------------------------------ 1. exports
def test_fav_yuv_h_is_exported_and_fav_h_declares_what_it_declared(favlib):
    declared = _declared("fav_yuv.h")
    assert len(declared) == 7 and "fav_stream_encode_yuv_layout" in declared
    L = favlib.lib()
    for name in declared:
        assert hasattr(L, name), f"libfav.so does not export {name}"
    assert declared == set(favlib.EXPORTS_YUV)
    old = _declared("fav.h")
    assert len(old) == 117 and old == set(favlib.EXPORTS) and not (old & declared)


# ------------------------------------------------------------------------------------------------ 2. headers
TAGS = [("C420", 0, 0, 8), ("C420jpeg", 0, 0, 8), ("C420mpeg2", 0, 1, 8), ("C444", 1, 0, 8), ("C422", 2, 1, 8)] + \
       [(f"C{b}p{n}", c, s, n) for b, c, s in (("420", 0, 0), ("422", 2, 1), ("444", 1, 0)) for n in DEEP]


@pytest.mark.parametrize("tag,chroma,siting,depth", TAGS, ids=[t[0] for t in TAGS])
def test_every_accepted_c_tag_parses_and_survives_format_then_parse(favlib, tag, chroma, siting, depth):
    h = favlib.y4m_parse_stream_header(f"YUV4MPEG2 W64 H48 F30000:1001 Ip A1:1 {tag} XCOLORRANGE=FULL XA=b\n".encode())
    lay = h.layout
    assert (lay.struct_bytes, lay.chroma, lay.siting, lay.depth, lay.matrix, lay.full_range) == (24, chroma, siting, depth, favlib.YUV_BT601, 1)
    line = favlib.y4m_format_stream_header(h)
    want_tag = "C420jpeg" if tag == "C420" else tag
    assert line == f"YUV4MPEG2 W64 H48 F30000:1001 Ip A1:1 {want_tag} XCOLORRANGE=FULL XA=b\n".encode()
    back = favlib.y4m_parse_stream_header(line)
    for name, _ in favlib.Y4mStreamHeader._fields_:
        a, b = getattr(h, name), getattr(back, name)
        if name == "layout":
            a, b = [tuple(getattr(x, f) for f, _ in favlib.YuvLayout._fields_) for x in (a, b)]
        assert a == b, (name, a, b)


@pytest.mark.parametrize("tag", ["C420paldv", "C411", "Cmono", "Cmono16", "C444alpha", "C420p11", "C422p8", "C444p15", "C420p", "C420p100", "It", "Ib", "Im"])
def test_stream_header_refusals_name_the_tag(favlib, tag):
    with pytest.raises(favlib.FavError) as e:
        favlib.y4m_parse_stream_header(f"YUV4MPEG2 W64 H48 F25:1 {tag} A1:1\n".encode())
    assert tag in str(e.value) and "error -4" in str(e.value), str(e.value)


def test_stream_header_malformed_is_einval(favlib):
    for line, what in ((b"YUV4MPEG2 H48 C422p10\n", "W tag is missing"), (b"YUV4MPEG W64 H48\n", "YUV4MPEG2"),
                       (b"YUV4MPEG2 W64 H48 C422 " + b"X" * 1100 + b"\n", "longer than 1024"), (b"YUV4MPEG2 W6x4 H48\n", "W6x4"),
                       (b"YUV4MPEG2 W64 H48 Q1\n", "Q1"), (b"YUV4MPEG2 W64 H48 XCOLORRANGE=WIDE\n", "XCOLORRANGE=WIDE")):
        with pytest.raises(favlib.FavError) as e:
            favlib.y4m_parse_stream_header(line)
        assert what in str(e.value) and "error -1" in str(e.value), (line[:40], str(e.value))


def test_formatter_refuses_what_the_grammar_cannot_say(favlib):
    h = favlib.y4m_parse_stream_header(b"YUV4MPEG2 W8 H8 C422p10\n")
    h.layout.siting = favlib.YUV_SITING_CENTER
    with pytest.raises(favlib.FavError) as e:
        favlib.y4m_format_stream_header(h)
    assert "error -4" in str(e.value) and "C422p10" in str(e.value)
    h = favlib.y4m_parse_stream_header(b"YUV4MPEG2 W8 H8 C420p10\n")
    h.layout.siting = favlib.YUV_SITING_LEFT
    with pytest.raises(favlib.FavError) as e:
        favlib.y4m_format_stream_header(h)
    assert "error -4" in str(e.value) and "C420p10" in str(e.value)
    h.layout.siting, h.layout.depth = favlib.YUV_SITING_CENTER, 11
    with pytest.raises(favlib.FavError) as e:
        favlib.y4m_format_stream_header(h)
    assert "error -1" in str(e.value) and "depth must be" in str(e.value)


@pytest.mark.parametrize("line", [
    b"YUV4MPEG2 XYSCSS=420MPEG2 A128:117 C420mpeg2 H1080 Ip F30000:1001 XCOLORRANGE=FULL W1920 XFOO=a:b\n",
    b"YUV4MPEG2 W640 H480\n", b"YUV4MPEG2 W4 H2 C444\nFRAME\n", b"YUV4MPEG2 W1280 H720 C420 I? XCOLORRANGE=LIMITED", b"YUV4MPEG2 W8 H8 C420jpeg XA=1"])
def test_both_parsers_agree_on_what_the_old_one_accepts(favlib, line):
    a, b = favlib.y4m_parse_header(line), favlib.y4m_parse_stream_header(line)
    for name in ("W", "H", "fps_num", "fps_den", "aspect_num", "aspect_den", "interlace", "xtags"):
        assert getattr(a, name) == getattr(b, name), name
    assert (a.fmt.chroma, a.fmt.siting, a.fmt.matrix, a.fmt.full_range) == (b.layout.chroma, b.layout.siting, b.layout.matrix, b.layout.full_range)
    assert b.layout.depth == 8
    assert favlib.y4m_format_header(a) == favlib.y4m_format_stream_header(b)


# ------------------------------------------------------------------------------------------------ 3. frame bytes
def test_layout_frame_bytes_and_field_checks_need_no_device(favlib):
    for (c, s), d in itertools.product(M.SAMPLINGS, M.DEPTHS):
        lay = M.Layout(c, s, "709", False, d)
        for w, h in ((1, 1), (5, 3), (64, 48), (1279, 719)):
            assert favlib.yuv_layout_frame_bytes(w, h, _clayout(favlib, lay)) == M.frame_bytes(w, h, lay), (lay, w, h)
    assert M.frame_bytes(5, 3, M.Layout("422", "left", "601", False, 10)) == 2 * (15 + 2 * 3 * 3)
    ok = M.Layout()
    for w, h, cl, msg in ((4, 4, _clayout(favlib, ok, struct_bytes=16), "struct_bytes must be"), (4, 4, _clayout(favlib, ok, struct_bytes=0), "struct_bytes must be"),
                          (4, 4, favlib.yuv_layout(chroma=3), "chroma must be"), (4, 4, favlib.yuv_layout(siting=2), "siting must be"),
                          (4, 4, favlib.yuv_layout(chroma=favlib.YUV_422, siting=-1), "siting must be"),
                          (4, 4, favlib.yuv_layout(matrix=2), "matrix must be"), (4, 4, favlib.yuv_layout(depth=11), "depth must be"),
                          (4, 4, favlib.yuv_layout(depth=7), "depth must be"), (4, 4, favlib.yuv_layout(depth=17), "depth must be"),
                          (0, 4, favlib.yuv_layout(), "bad frame size"), (1 << 14, (1 << 14) + 1, favlib.yuv_layout(), "bad frame size")):
        with pytest.raises(favlib.FavError) as e:
            favlib.yuv_layout_frame_bytes(w, h, cl)
        assert msg in str(e.value), str(e.value)
    assert favlib.yuv_layout_frame_bytes(4, 4, favlib.yuv_layout(chroma=favlib.YUV_444, siting=3, depth=16)) == 96        # the siting of 4:4:4 is not read


# ------------------------------------------------------------------------------------------------ 4. the model
def _cube():
    """every combination of 14 values per channel (the corners of the RGB cube among them), as an image [196][14][3]"""
    v = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 240, 254, 255], np.uint8)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 14, 3)


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(21)
    return [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8), _cube()]


def _lsb(a, b):
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max())


@pytest.mark.parametrize("depth", M.DEPTHS)
def test_fp32_model_within_one_sample_of_fp64_both_directions(images, depth):
    """Measured on the model, all four (matrix, range) pairs, 4:4:4, random bytes plus the cube / random 16-bit samples: the fp32 model
    differs from its fp64 form by at most 1 sample (encode) and 1 byte (decode) at every depth 8, 9, 10, 12, 14, 16 -- a rounding
    boundary falling between the two, never more.  Asserted at that bound."""
    rng = np.random.default_rng(depth)
    for m, r in itertools.product(("601", "709"), (False, True)):
        lay = M.Layout("444", "center", m, r, depth)
        for img in images:
            assert _lsb(M.rgb_to_yuv(img, lay, np.float32), M.rgb_to_yuv(img, lay, np.float64)) <= 1
        f32 = rng.uniform(-0.2, 1.2, (3, 64, 64)).astype(np.float32)
        assert _lsb(M.rgb_f32_to_yuv(f32, lay, np.float32), M.rgb_f32_to_yuv(f32, lay, np.float64)) <= 1
        planes = rng.integers(0, 1 << (8 if depth == 8 else 16), 3 * 128 * 128).astype(M.sample_dtype(lay))       # every value a sample can hold
        assert _lsb(M.yuv_to_rgb(planes, 128, 128, lay, np.float32), M.yuv_to_rgb(planes, 128, 128, lay, np.float64)) <= 1


@pytest.mark.parametrize("depth", M.DEPTHS)
def test_444_round_trip_returns_every_byte_from_depth_10_on(images, depth):
    """RGB8 -> 4:4:4 at depth D -> RGB8, fp32 model, random bytes plus the cube with its corners.  Measured: depth 8 loses up to 1 (full
    range) / 2 (limited) grey levels, as yuv_model's own round trip; depth 9 up to 1; from depth 10 on every byte comes back, in both
    ranges and both matrices.  Asserted at those bounds."""
    bound = {8: (1, 2), 9: (1, 1)}.get(depth, (0, 0))
    for m, r in itertools.product(("601", "709"), (False, True)):
        lay = M.Layout("444", "center", m, r, depth)
        for img in images:
            h, w = img.shape[:2]
            assert _lsb(M.yuv_to_rgb(M.rgb_to_yuv(img, lay), w, h, lay), img) <= bound[0 if r else 1], (lay,)


def test_depth_8_is_the_8_bit_model():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    f32 = rng.uniform(-0.2, 1.2, (3, 7, 9)).astype(np.float32)
    for f in M8.ALL_FORMATS:
        lay = M.Layout(f.chroma, f.siting, f.matrix, f.full_range, 8)
        for k, v in M8.constants(f).items():
            assert M.constants(lay)[k] == v and M.constants(lay)[k].dtype == np.float32
        enc = M8.rgb_to_yuv(img, f)
        assert np.array_equal(M.rgb_to_yuv(img, lay), enc) and np.array_equal(M.rgb_f32_to_yuv(f32, lay), M8.rgb_f32_to_yuv(f32, f))
        assert np.array_equal(M.yuv_to_rgb(enc, 9, 7, lay), M8.yuv_to_rgb(enc, 9, 7, f))


@pytest.mark.parametrize("siting,want", [("center", lambda x: 2 * x - 1), ("left", lambda x: 2 * x)])
def test_422_siting_and_no_vertical_step(siting, want):
    C = (4 * np.arange(20)[None, :] + 1000 * np.arange(5)[:, None]).astype(np.uint16)          # C[y][j] = 4 j + 1000 y
    up = M.upsample_422(C, 40, siting)
    x = np.arange(1, 39)
    assert np.array_equal(up[:, 1:39], (want(x)[None, :] + 1000 * np.arange(5)[:, None]).astype(np.float32))
    # a ramp along x comes back through the reduction where the siting says it sits; rows stay apart
    ramp = np.broadcast_to(np.arange(40, dtype=np.float32), (5, 40)) + 100 * np.arange(5, dtype=np.float32)[:, None]
    down = M.downsample_422(ramp, siting)
    assert down.shape == (5, 20)
    assert np.array_equal(down[:, 1:19], (2 * np.arange(1, 19) + (0.5 if siting == "center" else 0.0))[None, :] + 100 * np.arange(5)[:, None])


@pytest.mark.parametrize("depth", DEEP)
def test_limited_range_deep_planes_of_an_8_bit_frame_decode_to_its_bytes(depth):
    """samples x 2^(D-8) with limited-range constants x 2^(D-8): a power of two commutes with every rounding, so the fp32 model gives
    the 8-bit frame's RGB bytes exactly -- for every sampling, both matrices, random bytes over the whole range"""
    rng = np.random.default_rng(depth)
    w, h = 19, 7
    for (c, s), m in itertools.product(M.SAMPLINGS, ("601", "709")):
        l8, ld = M.Layout(c, s, m, False, 8), M.Layout(c, s, m, False, depth)
        p8 = rng.integers(0, 256, M.frame_samples(w, h, l8)).astype(np.uint8)
        pd = p8.astype(np.uint16) << (depth - 8)
        assert np.array_equal(M.yuv_to_rgb(pd, w, h, ld), M.yuv_to_rgb(p8, w, h, l8)), (ld,)


def test_f32_source_truncates_at_depth_8_only():
    x = np.array([-0.5, 0.0, 0.25, 100.7 / 255, 0.999, 1.0, 7.0], np.float32)
    img = np.broadcast_to(x, (3, 2, 7)).copy()
    l8, l10 = M.Layout("444", "center", "601", True, 8), M.Layout("444", "center", "601", True, 10)
    y8 = M.split_planes(M.rgb_f32_to_yuv(img, l8), 7, 2, l8)[0][0]
    y10 = M.split_planes(M.rgb_f32_to_yuv(img, l10), 7, 2, l10)[0][0]
    assert y8.tolist() == [0, 0, 63, 100, 254, 255, 255]                      # image.save's bytes
    assert y10.tolist() == [0, 0, 256, 404, 1022, 1023, 1023]                  # grey: Y = clamp(x) * 1023, rounded once
    assert y10.dtype == np.uint16 and M.payload(y10, l10).size == 14


# ------------------------------------------------------------------------------------------------ 5. fav_stylize: refused before a device is opened
@pytest.mark.parametrize("args,msg", [
    (["-input_y4m", "x.y4m", "-output_y4m", "y.y4m", "-y4m_pixel_format", "420p11"], "-y4m_pixel_format must be 420jpeg, 420mpeg2, 422, 444"),
    (["-input_y4m", "x.y4m", "-output_y4m", "y.y4m", "-y4m_pixel_format", "420"], "-y4m_pixel_format must be"),
    (["-input_y4m", "x.y4m", "-output_y4m", "y.y4m", "-y4m_pixel_format", "420paldv"], "-y4m_pixel_format must be"),
    (["-input_y4m", "x.y4m", "-output_y4m", "y.y4m", "-y4m_pixel_format", "422p10", "-y4m_format", "444"], "-y4m_format and -y4m_pixel_format both"),
    (["-input_y4m", "x.y4m", "-output_y4m", "y.y4m", "-y4m_pixel_format", "420p10", "-original_colors", "1"], "output format 420p10"),
    (["-input_y4m", "x.y4m", "-output_y4m", "y.y4m", "-y4m_pixel_format", "422", "-original_colors", "1"], "output format 422"),
    (["-input_y4m", "x.y4m", "-output_y4m", "y.y4m", "-y4m_format", "422"], "-y4m_format must be"),
])
def test_fav_stylize_refuses_before_the_device(favlib, args, msg):
    r = subprocess.run([STYLIZE] + args + ["-estimate_flow", "1"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert r.returncode != 0 and msg in r.stderr, r.stderr
    assert "HIP" not in r.stderr and r.stdout == ""


def test_fav_stylize_dry_run_prints_the_outputs_tag(favlib):
    import json
    for extra, want in ((["-y4m_pixel_format", "422p10"], "422p10"), (["-y4m_format", "420mpeg2"], "420mpeg2"), ([], "input")):
        r = subprocess.run([STYLIZE, "-input_y4m", "x.y4m", "-output_y4m", "y.y4m", "-estimate_flow", "1", "-dry_run", "1"] + extra,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout.strip().splitlines()[-1])["streams"][0]["output_y4m_tag"] == want
    r = subprocess.run([STYLIZE, "-input_pattern", "f_%05d.ppm", "-output_y4m", "y.y4m", "-estimate_flow", "1", "-dry_run", "1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1])["streams"][0]["output_y4m_tag"] == "420jpeg"
