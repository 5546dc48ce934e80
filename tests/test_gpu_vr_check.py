"""The 360-degree path with the forward-backward consistency check on the GPU (fav_vr_face_flow / fav_vr_prefetch_mask): the check,
the border max and everything behind them must give the bits of the certainty-FILE path (fav_vr_face) fed with the mask the
stand-alone operator (fav_consistency_u8) computes from the same flows, and the mask itself must be the CPU oracle's -- the
restatement of the reference's consistencyChecker that tests/test_cpu_oracle.py pins on the reference binary.

Why bit equality can be asked of the network's faces too: everything downstream of the certainty plane is the same kernels on the same
bits, and the file path reproduces its own faces bit for bit from run to run (test_file_path_reproduces_itself checks that premise
on two independent objects; observed equal on an MI355X).

Fixture recipe of test_gpu_vr.py::test_vr_two_frames_vs_oracle: tests/golden/tiny_model.t7, 64x64 faces, overlap 24, two frames, synth
flows (tests/util/vr_check_inputs.py; every compared mask has 10..90 % of its bytes at 255 on the oracle, tests/test_cpu_vr_check.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest


sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import vr_check_inputs as VI  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
KW = dict(overlap_w=VI.OVERLAP, overlap_h=VI.OVERLAP, out_equi_w=96, out_equi_h=48, seed=7, fill_random=True, median=3)


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a is not None else None


def _file_path(favlib, net, cuda, inputs, structure, hp=VI.HP):
    """the certainty-file path on the operator's masks: per face (mask, get(5), face), per frame (equi u8, cube u8)"""
    vr = favlib.VR(net, hp, hp, **KW)
    faces, frames = [], []
    for (i, f, bw, fw) in inputs:
        F, B, Fw = T(f, cuda), T(bw, cuda), T(fw, cuda)
        mask = favlib.consistency(B, Fw, F if structure else None) if bw is not None else None
        out = vr.face(i, F, B, mask)
        faces.append((mask.cpu().numpy() if mask is not None else None, vr.get(5).cpu().numpy() if i > 1 else None, out.cpu().numpy()))
        if (i - 1) % 6 == 5:
            frames.append(tuple(x.cpu().numpy() for x in vr.finish_frame()))
    return faces, frames


@pytest.fixture(scope="module")
def net(favlib, golden_dir):
    return favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0)


@pytest.fixture(scope="module")
def inputs():
    return VI.face_inputs()


@pytest.fixture(scope="module")
def baseline(favlib, net, cuda, inputs):
    return {s: _file_path(favlib, net, cuda, inputs, s) for s in (0, 1)}


def _compare_face(vr, got, want, i, structure):
    mask, cert, face = want
    if mask is not None:
        np.testing.assert_array_equal(vr.last_mask().cpu().numpy(), mask, err_msg=f"mask of face {i}, structure {structure}")
    if cert is not None:
        np.testing.assert_array_equal(vr.get(5).cpu().numpy(), cert, err_msg=f"certainty plane of face {i}")
    np.testing.assert_array_equal(got.cpu().numpy(), face, err_msg=f"face {i}")


def _compare_frame(vr, want):
    e, c = vr.finish_frame()
    np.testing.assert_array_equal(e.cpu().numpy(), want[0])
    np.testing.assert_array_equal(c.cpu().numpy(), want[1])


def test_file_path_reproduces_itself(favlib, net, cuda, inputs, baseline):
    """the premise of the bit comparisons below: fav_vr_face twice on identical inputs, two independent objects"""
    faces, frames = _file_path(favlib, net, cuda, inputs, 1)
    for (m, c, f), (m0, c0, f0) in zip(faces, baseline[1][0]):
        np.testing.assert_array_equal(f, f0)
    for a, b in zip(frames, baseline[1][1]):
        np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])


@pytest.mark.parametrize("structure", [0, 1], ids=["3arg", "4arg"])
def test_face_flow_equals_file_path_bit_for_bit(favlib, net, cuda, inputs, baseline, structure):
    """test 1: every face of two frames; mask, certainty after border max + erosion, the network's face and the frame's two u8 images"""
    faces, frames = baseline[structure]
    vr = favlib.VR(net, VI.HP, VI.HP, **KW)
    for k, (i, f, bw, fw) in enumerate(inputs):
        got = vr.face_flow(i, T(f, cuda), T(bw, cuda), T(fw, cuda), structure)
        _compare_face(vr, got, faces[k], i, structure)
        if (i - 1) % 6 == 5:
            _compare_frame(vr, frames[i // 6 - 1])
    # the two modes are different masks on these inputs (the structure term decides pixels): the parametrisation is not vacuous
    assert any((a[0] != b[0]).any() for a, b in zip(baseline[0][0], baseline[1][0]) if a[0] is not None)


@pytest.mark.parametrize("structure", [0, 1], ids=["3arg", "4arg"])
def test_mask_equals_cpu_oracle(favlib, oracle, net, cuda, inputs, structure):
    """test 2: zero bytes may differ from the oracle's checker; both byte values occur in every compared mask (10..90 % at 255)"""
    vr = favlib.VR(net, VI.HP, VI.HP, **KW)
    compared = 0
    for (i, f, bw, fw) in inputs:
        vr.face_flow(i, T(f, cuda), T(bw, cuda), T(fw, cuda), structure)
        if bw is not None:
            want = oracle.consistency(bw, fw, f if structure else None)
            assert 0.10 <= VI.reliable_fraction(want) <= 0.90, (i, VI.reliable_fraction(want))
            got = vr.last_mask().cpu().numpy()
            assert int((got != want).sum()) == 0, f"face {i}: {int((got != want).sum())} bytes differ from the oracle"
            compared += 1
        if (i - 1) % 6 == 5:
            vr.finish_frame()
    assert compared == 6


@pytest.mark.parametrize("structure", [0, 1], ids=["3arg", "4arg"])
def test_face_76_not_a_multiple_of_16(favlib, net, cuda, structure):
    """test 3a: 76x76 faces (a multiple of 4, not of 16 or 32: ragged tiles, padded row pitches of the structure planes), modes 0, 3, 5"""
    hp = 76
    inputs = VI.face_inputs(hp, hp)
    faces, _ = _file_path(favlib, net, cuda, inputs, structure, hp)
    vr = favlib.VR(net, hp, hp, **KW)
    for k, (i, f, bw, fw) in enumerate(inputs):
        got = vr.face_flow(i, T(f, cuda), T(bw, cuda), T(fw, cuda), structure)
        if i >= 7 and (i - 1) % 6 in (0, 3, 5):
            _compare_face(vr, got, faces[k], i, structure)
        if (i - 1) % 6 == 5:
            vr.finish_frame()


def test_extreme_flows(favlib, net, cuda, inputs, golden_dir):
    """test 3b: NaN, +-inf and |flow| >= 2^31 (tests/golden/mask_extreme_flows_24x40.npz tiled into a face-sized field): the fused kernel
    must take the range test of consistency_pixel.h, i.e. give the operator's mask, and gather nothing out of bounds"""
    g = np.load(os.path.join(golden_dir, "mask_extreme_flows_24x40.npz"))
    bw = np.ascontiguousarray(np.tile(g["bw"], (3, 2, 1))[:VI.HP, :VI.HP]); fw = np.ascontiguousarray(np.tile(g["fw"], (3, 2, 1))[:VI.HP, :VI.HP])
    assert not np.isfinite(bw).all() and np.abs(bw[np.isfinite(bw)]).max() >= 2.0 ** 31
    f = inputs[6][1]
    for structure in (0, 1):
        want = favlib.consistency(T(bw, cuda), T(fw, cuda), T(f, cuda) if structure else None).cpu().numpy()
        vr = favlib.VR(net, VI.HP, VI.HP, **KW)
        for (i, fr, _, _) in inputs[:6]:
            vr.face_flow(i, T(fr, cuda))
        vr.finish_frame()
        vr.face_flow(7, T(f, cuda), T(bw, cuda), T(fw, cuda), structure)
        np.testing.assert_array_equal(vr.last_mask().cpu().numpy(), want)
        assert (want == 0).any() and (want == 255).any()


@pytest.mark.parametrize("structure", [0, 1], ids=["3arg", "4arg"])
def test_look_ahead_masks(favlib, net, cuda, inputs, baseline, structure):
    """test 4: all six masks of frame 2 started ahead on the side stream, then the six faces: the bits of test 1.  A look-ahead for a face
    of the first frame is a no-op; one whose pointers are not the face's is discarded and the face computes from what it was passed."""
    faces, frames = baseline[structure]
    vr = favlib.VR(net, VI.HP, VI.HP, **KW)
    dev = [(i, T(f, cuda), T(bw, cuda), T(fw, cuda)) for (i, f, bw, fw) in inputs]
    vr.prefetch_mask(1, dev[0][1], None, None, structure)             # i < 7: FAV_OK, nothing happens (no flows to read)
    assert favlib.lib().fav_vr_prefetch_mask(vr.h, 3, favlib._p(dev[2][1]), None, None, structure, favlib._stream()) == 0
    for (i, F, B, Fw) in dev[:6]:
        got = vr.face_flow(i, F, B, Fw, structure)
        np.testing.assert_array_equal(got.cpu().numpy(), faces[i - 1][2])
    _compare_frame(vr, frames[0])
    for (i, F, B, Fw) in dev[6:]:
        vr.prefetch_mask(i, F, B, Fw, structure)
    for (i, F, B, Fw) in dev[6:]:
        got = vr.face_flow(i, F, B, Fw, structure)
        _compare_face(vr, got, faces[i - 1], i, structure)
    _compare_frame(vr, frames[1])
    # a third frame on the second frame's inputs: face 13's look-ahead is made with OTHER flows (face 14's); the face must not use it
    other = favlib.VR(net, VI.HP, VI.HP, **KW)                         # the same three frames without any look-ahead
    for (i, F, B, Fw) in dev:
        other.face_flow(i, F, B, Fw, structure)
        if (i - 1) % 6 == 5:
            other.finish_frame()
    _, F, B, Fw = dev[6]
    want = other.face_flow(13, F, B, Fw, structure)
    vr.prefetch_mask(13, F, dev[7][2], dev[7][3], structure)
    got = vr.face_flow(13, F, B, Fw, structure)
    np.testing.assert_array_equal(vr.last_mask().cpu().numpy(), other.last_mask().cpu().numpy())
    np.testing.assert_array_equal(vr.last_mask().cpu().numpy(), faces[6][0])
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    # ... and a look-ahead in the other mode is not this face's either
    vr.prefetch_mask(14, dev[7][1], dev[7][2], dev[7][3], 1 - structure)
    vr.face_flow(14, dev[7][1], dev[7][2], dev[7][3], structure)
    np.testing.assert_array_equal(vr.last_mask().cpu().numpy(), faces[7][0])


def test_errors(favlib, net, cuda, inputs):
    """test 5"""
    vr = favlib.VR(net, VI.HP, VI.HP, **KW)
    i, f, bw, fw = inputs[6]
    F, B, Fw = T(f, cuda), T(bw, cuda), T(fw, cuda)
    # before the previous frame is finished: the error of fav_vr_face
    with pytest.raises(favlib.FavError, match=r"libfav error -1: fav_vr_face: face 7 needs the flow, the certainty and a finished previous frame") as e_file:
        vr.face(7, F, B, favlib.consistency(B, Fw))
    with pytest.raises(favlib.FavError, match=r"libfav error -1: fav_vr_face_flow: face 7 needs the flow, the certainty and a finished previous frame") as e_flow:
        vr.face_flow(7, F, B, Fw, 0)
    assert str(e_flow.value).replace("fav_vr_face_flow", "fav_vr_face") == str(e_file.value)
    for (k, fr, _, _) in inputs[:6]:
        vr.face_flow(k, T(fr, cuda))
    vr.finish_frame()
    with pytest.raises(favlib.FavError, match=r"libfav error -1: .*face 7 .*forward"):         # FAV_EINVAL, naming the face
        vr.face_flow(7, F, B, None, 0)
    with pytest.raises(favlib.FavError, match=r"libfav error -1: .*face 7 "):
        vr.prefetch_mask(7, F, B, None, 0)
    vr.face_flow(7, F, B, Fw, 0)                                        # the object is still usable


def _write_vr_clip(oracle, d, inputs):
    import vr_oracle as V
    for (i, f, bw, fw) in inputs:
        fr, face = (i - 1) // 6 + 1, V.PROC_ORDER[(i - 1) % 6]
        oracle.write_pnm(str(d / f"frame_{fr:05d}-{face}.ppm"), f)
        if bw is not None:
            os.makedirs(d / f"flow-{face}", exist_ok=True)
            oracle.write_flo(str(d / f"flow-{face}" / f"backward_{fr}_{fr-1}.flo"), bw)
            oracle.write_flo(str(d / f"flow-{face}" / f"forward_{fr-1}_{fr}.flo"), fw)


@pytest.mark.parametrize("structure", [1, 0], ids=["4arg", "3arg"])
def test_cli_forward_flow_equals_certainty_files(oracle, favlib, tmp_path, golden_dir, inputs, monkeypatch, structure):
    """test 6: bin/fav_stylize_vr with -occlusions_pattern on files bin/consistencyChecker wrote, against -forward_flow_pattern
    -structure <s>: byte-identical PNGs"""
    import vr_oracle as V
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import e2e_content
    monkeypatch.setenv("FAV_CC_DAEMON", "0")                             # the process-per-call form of the checker
    _write_vr_clip(oracle, tmp_path, inputs)
    for (i, f, bw, fw) in inputs[6:]:
        face = V.PROC_ORDER[(i - 1) % 6]
        fl = tmp_path / f"flow-{face}"
        cmd = [os.path.join(BIN, "consistencyChecker"), str(fl / "backward_2_1.flo"), str(fl / "forward_1_2.flo"), str(fl / "reliable_2_1.pgm")]
        if structure:
            cmd.append(str(tmp_path / f"frame_00002-{face}.ppm"))
        assert subprocess.run(cmd, capture_output=True).returncode == 0
    e2e_content.age_files(str(tmp_path))
    base = [os.path.join(BIN, "fav_stylize_vr"), "-input_pattern", str(tmp_path / "frame_%05d-%d.ppm"),
            "-flow_pattern", str(tmp_path / "flow-%d" / "backward_[%d]_{%d}.flo"), "-gpu", "0",
            "-model_vid", os.path.join(golden_dir, "tiny_model.t7"), "-model_img", "self", "-overlap_pixel_h", "24", "-overlap_pixel_w", "24",
            "-out_equi", "-out_equi_w", "96", "-out_equi_h", "48", "-out_cubemap", "-fill_occlusions", "uniform-random", "-seed", "9"]
    runs = {"file": ["-occlusions_pattern", str(tmp_path / "flow-%d" / "reliable_[%d]_{%d}.pgm")],
            "flow": ["-forward_flow_pattern", str(tmp_path / "flow-%d" / "forward_{%d}_[%d].flo"), "-structure", str(structure)]}
    for name, extra in runs.items():
        r = subprocess.run(base + extra + ["-output_prefix", str(tmp_path / name / "out")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    for fr in (1, 2):
        for kind in ("equi", "cubemap"):
            a = open(tmp_path / "file" / f"out-{fr:05d}_{kind}.png", "rb").read()
            b = open(tmp_path / "flow" / f"out-{fr:05d}_{kind}.png", "rb").read()
            assert len(a) > 100 and a == b, (fr, kind)
