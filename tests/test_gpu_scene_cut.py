"""-scene_cut on the GPU: fav_scene_change_rgb8 EQUAL to the integer numpy model (tests/util/scene_model.py) in all 17 numbers -- uneven
cells, rows shorter than a wide load, odd pitches, constant frames, unaligned buffers, a host-mapped result, a reused workspace -- and
fav_stylize -scene_cut on a six-frame clip with one cut: the log, and the frames behind the cut byte-equal to those of a clip that starts
there."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import scene_model as S  # noqa: E402
import yuv_model as M  # noqa: E402

from fav_amd import t7  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
# (W, H): one pixel per cell; uneven cells and rows shorter than one 48-byte load; an odd row pitch; more than one workgroup (4096 pixels each)
SIZES = [(4, 4), (13, 7), (67, 35), (256, 64)]
PATTERN = 0x5A5A5A5A


def _const(w, h, rgb):
    a = np.empty((h, w, 3), np.uint8)
    a[...] = rgb
    return a


@pytest.fixture(scope="module")
def cases():
    """per size the input pairs and the model's 17 numbers, computed once"""
    out = {}
    for w, h in SIZES:
        rng = np.random.default_rng(100 * w + h)
        noise = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        pairs = {"noise": noise, "black-black": (_const(w, h, (0, 0, 0)), _const(w, h, (0, 0, 0))),
                 "constant-other-colour": (_const(w, h, (10, 200, 30)), _const(w, h, (250, 20, 90)))}
        out[(w, h)] = {k: (a, b, S.scene_change(a, b)) for k, (a, b) in pairs.items()}
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_operator_equals_the_model_in_all_17_integers(favlib, cuda, cases, size):
    import torch
    w, h = size
    for name, (a, b, want) in cases[size].items():
        ta, tb = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
        got = favlib.scene_change(ta, tb)
        assert got == want, f"{name} {w}x{h}: {got} != {want}"
        assert favlib.scene_change(ta, ta) == (0, [0] * 16), f"{name} {w}x{h}: prev is cur"
    a, b, want = cases[size]["constant-other-colour"]
    assert want[0] == 2 * w * h                                      # (the two colours' lumas fall in different bins: every pixel counts twice)


def test_frames_at_byte_offsets_1_and_3(favlib, cuda, cases):
    """no alignment is required of the frames, and nothing outside them is read: the bytes around them differ between the calls"""
    import torch
    w, h = 67, 35
    a, b, want = cases[(w, h)]["noise"]
    n = w * h * 3
    for off, fill in ((1, 0), (3, 255)):
        bufs = []
        for src in (a, b):
            t = torch.full((n + 8,), fill, dtype=torch.uint8, device=cuda)
            t[off:off + n] = torch.from_numpy(src).to(cuda).reshape(-1)
            bufs.append(t)
        got = favlib.scene_change(bufs[0][off:off + n].view(h, w, 3), bufs[1][off:off + n].view(h, w, 3))
        assert got == want, f"offset {off}"


def test_result_in_host_mapped_memory(favlib, cuda, cases):
    import torch
    w, h = 256, 64
    a, b, want = cases[(w, h)]["noise"]
    res = torch.full((17,), 0x5A5A5A5A, dtype=torch.int32).pin_memory()
    got = favlib.scene_change(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), result=res)
    assert got == want
    assert (int(res[0]) & 0xFFFFFFFF, [int(v) & 0xFFFFFFFF for v in res[1:]]) == want


def test_workspace_is_zeroed_by_the_call(favlib, cuda, cases):
    """the same workspace, first full of garbage, then holding the previous call's table: the same numbers every time"""
    import torch
    w, h = 67, 35
    a, b, want = cases[(w, h)]["noise"]
    ta, tb = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)
    ws = torch.full((favlib.scene_change_workspace_bytes(),), 0xA5, dtype=torch.uint8, device=cuda)
    for _ in range(3):
        assert favlib.scene_change(ta, tb, workspace=ws) == want
    a2, b2, want2 = cases[(w, h)]["constant-other-colour"]
    assert favlib.scene_change(torch.from_numpy(a2).to(cuda), torch.from_numpy(b2).to(cuda), workspace=ws) == want2
    assert favlib.scene_change(ta, tb, workspace=ws) == want


def test_bad_arguments_are_einval_and_write_nothing(favlib, cuda):
    import torch
    res = torch.full((17,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    ws = torch.full((favlib.scene_change_workspace_bytes(),), 0xA5, dtype=torch.uint8, device=cuda)
    a = torch.zeros((8, 8, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(favlib.FavError) as e:
        favlib.scene_change(a, a, workspace=ws, result=res, w=3, h=8)            # W = 3
    assert "error -1" in str(e.value) and "3x8" in str(e.value)
    with pytest.raises(favlib.FavError) as e:
        favlib.scene_change(a, a, workspace=ws, result=res, w=8, h=3)
    assert "error -1" in str(e.value)
    with pytest.raises(favlib.FavError) as e:
        favlib.scene_change(a, a, workspace=ws, result=res, workspace_bytes=favlib.scene_change_workspace_bytes() - 1)
    assert "error -1" in str(e.value) and "workspace" in str(e.value)
    torch.cuda.synchronize()
    assert (res == 0x5A5A5A5A).all() and (ws == 0xA5).all(), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ the CLI
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _run(args, **kw):
    return subprocess.run([STYLIZE] + args, capture_output=True, timeout=300, **kw)


def _log(path):
    """[(index, total, score, cut)]"""
    rows = [ln.split() for ln in open(path).read().splitlines()]
    assert all(len(r) == 4 for r in rows), rows
    return [(int(r[0]), int(r[1]), float(r[2]), int(r[3])) for r in rows]


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """the six frames as PPM files (six/), frames 4-6 as a clip of their own (tail/), a video model and a DIFFERENT image model"""
    d = tmp_path_factory.mktemp("scene_cut")
    frames = S.cut_clip()
    for sub, fr in (("six", frames), ("tail", frames[3:])):
        (d / sub).mkdir()
        for i, f in enumerate(fr):
            S.write_ppm(str(d / sub / f"frame_{i + 1:05d}.ppm"), f)
    t7.make_synthetic_checkpoint(str(d / "vid.t7"), arch="c9s1-8,d16,d32,R32,R32,u16,u8,c9s1-3", seed=3)
    t7.make_synthetic_checkpoint(str(d / "img.t7"), arch="c9s1-8,d16,d32,R32,R32,u16,u8,c9s1-3", seed=5, in_channels=3)
    return d, frames


def _common(d):
    return ["-model_vid", str(d / "vid.t7"), "-model_img", str(d / "img.t7"), "-estimate_flow", "1", "-poll_settle", "0"]


def test_cli_cut_restarts_the_recurrence(favlib, clip):
    d, frames = clip
    cut = _run(["-input_pattern", str(d / "six" / "frame_%05d.ppm"), "-output_prefix", str(d / "cut" / "out"),
                "-scene_cut", "0.5", "-scene_cut_log", str(d / "cut" / "log.txt")] + _common(d))
    assert cut.returncode == 0, cut.stderr.decode()
    plain = _run(["-input_pattern", str(d / "six" / "frame_%05d.ppm"), "-output_prefix", str(d / "plain" / "out")] + _common(d))
    assert plain.returncode == 0, plain.stderr.decode()
    tail = _run(["-input_pattern", str(d / "tail" / "frame_%05d.ppm"), "-output_prefix", str(d / "tailout" / "out")] + _common(d))
    assert tail.returncode == 0, tail.stderr.decode()
    # the log: frame 4 and only frame 4 is a cut; the totals are the model's
    log = _log(d / "cut" / "log.txt")
    assert [r[0] for r in log] == [1, 2, 3, 4, 5, 6] and [r[3] for r in log] == [0, 0, 0, 1, 0, 0], log
    want = [0] + [S.scene_change(frames[k - 1], frames[k])[0] for k in range(1, 6)]
    assert [r[1] for r in log] == want, (log, want)
    for r in log:
        assert abs(r[2] - r[1] / (2.0 * S.CLIP_W * S.CLIP_H)) < 1e-6
    # behind the cut: the frames of a clip that starts there; in front of it: the frames of the run without the option
    for k in (1, 2, 3):
        assert np.array_equal(_png(d / "cut" / f"out-{k + 3:05d}.png"), _png(d / "tailout" / f"out-{k:05d}.png")), f"frame {k + 3}"
        assert open(d / "cut" / f"out-{k + 3:05d}.png", "rb").read() == open(d / "tailout" / f"out-{k:05d}.png", "rb").read(), f"frame {k + 3}"
        assert open(d / "cut" / f"out-{k:05d}.png", "rb").read() == open(d / "plain" / f"out-{k:05d}.png", "rb").read(), f"frame {k}"
    # the guard of this test: without the option frame 4 is another picture (the image model is another network, the prior is used)
    assert not np.array_equal(_png(d / "cut" / "out-00004.png"), _png(d / "plain" / "out-00004.png"))
    assert cut.stdout.count(b"stylizing frame independently") == 2 and plain.stdout.count(b"stylizing frame independently") == 1


def test_cli_scene_cut_0_is_the_run_without_the_option(favlib, clip):
    d, _ = clip
    off = _run(["-input_pattern", str(d / "six" / "frame_%05d.ppm"), "-output_prefix", str(d / "off" / "out"), "-scene_cut", "0"] + _common(d))
    assert off.returncode == 0, off.stderr.decode()
    if not (d / "plain").exists():
        plain = _run(["-input_pattern", str(d / "six" / "frame_%05d.ppm"), "-output_prefix", str(d / "plain" / "out")] + _common(d))
        assert plain.returncode == 0, plain.stderr.decode()
    for k in range(1, 7):
        assert open(d / "off" / f"out-{k:05d}.png", "rb").read() == open(d / "plain" / f"out-{k:05d}.png", "rb").read(), f"frame {k}"


def test_cli_cut_in_a_y4m_stream(favlib, clip):
    """4:4:4 planes through -input_y4m: the measure runs on the RGB frame the conversion kernel leaves on the device"""
    d, frames = clip
    f = M.Format("444", "center", "601", False)
    planes = [M.rgb_to_yuv(fr, f) for fr in frames]
    M.write_y4m(str(d / "clip.y4m"), M.y4m_header(S.CLIP_W, S.CLIP_H, f), planes)
    r = _run(["-input_y4m", str(d / "clip.y4m"), "-output_prefix", str(d / "y4m" / "out"), "-scene_cut", "0.5",
              "-scene_cut_log", str(d / "y4m" / "log.txt")] + _common(d))
    assert r.returncode == 0, r.stderr.decode()
    log = _log(d / "y4m" / "log.txt")
    assert [r_[3] for r_ in log] == [0, 0, 0, 1, 0, 0], log
    rgb = [M.yuv_to_rgb(p, S.CLIP_W, S.CLIP_H, f) for p in planes]
    assert [r_[1] for r_ in log] == [0] + [S.scene_change(rgb[k - 1], rgb[k])[0] for k in range(1, 6)]


def test_cli_cut_with_backward(favlib, clip):
    """-backward walks 6, 5, ..., 1: the first frame of scene A in that order is frame 3"""
    d, frames = clip
    r = _run(["-input_pattern", str(d / "six" / "frame_%05d.ppm"), "-output_prefix", str(d / "back" / "out"), "-backward", "-num_frames", "7",
              "-scene_cut", "0.5", "-scene_cut_log", str(d / "back" / "log.txt")] + _common(d))
    assert r.returncode == 0, r.stderr.decode()
    log = _log(d / "back" / "log.txt")
    assert [r_[0] for r_ in log] == [6, 5, 4, 3, 2, 1] and [r_[3] for r_ in log] == [0, 0, 0, 1, 0, 0], log
    assert [r_[1] for r_ in log] == [0] + [S.scene_change(frames[k + 1], frames[k])[0] for k in (4, 3, 2, 1, 0)]
