"""360 degrees from equirectangular frames on the GPU: the transform kernel (csrc/kernels_equi.hip) against its numpy model
(tests/util/equi_model.py), the round trip through the project's own cube -> equirectangular map, bin/fav_transform_vr against the
library, and fav_stylize_vr -input_equi_pattern against the file route made of fav_transform_vr, fav_flow and fav_stylize_vr.

Gate of the fp32 planes (the rule of test_gpu_scale.py): with e32 = max|M32 - M64| of the two CPU models on the same input,
max|GPU - M64| <= max(4 e32, 2^-22 * 255).  The u8 faces are within 1 LSB of the fp64 model's.  Nothing is measured against the code under
test.  Measured e32 / max|GPU - M64| per case are printed; the figures of one run are in DESIGN.md."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import equi_model as E  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
VID = os.path.join(ROOT, "tests", "golden", "tiny_model.t7")
BLOCK_W, BLOCK_H = 64, 4                 # the kernel's block: dim3(64, 4) (checked below against the source)
# (equi W, H; edge; overlap; supersample): the issue's three and whole blocks plus a row and a column
CASES = [(97, 41, 24, 0, 1), (192, 96, 48, 8, 2), (130, 64, 33, 10, 4), (256, 128, 2 * BLOCK_W + 1, 12, 2)]
_models = {}


def _image(ew, eh):
    if (ew, eh) == (E.RT["ew"], E.RT["eh"]):
        return E.sphere_image(ew, eh)
    return np.random.default_rng(ew * 1000 + eh).integers(0, 256, (eh, ew, 3), dtype=np.uint8)      # every tap counts


def _model(case):
    """the case's image and both models' faces, computed once"""
    if case not in _models:
        ew, eh, edge, ov, ss = case
        img = _image(ew, eh)
        _models[case] = (img, E.equi_to_faces(img, edge, edge, ov, ov, ss, np.float32), E.equi_to_faces(img, edge, edge, ov, ov, ss, np.float64))
    return _models[case]


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _gate(case, faces, planes, what):
    _, (_, p32), (f64, p64) = _model(case)
    e32 = float(np.abs(p32.astype(np.float64) - p64).max())
    bound = max(4 * e32, 2.0 ** -22 * 255)
    err = float(np.abs(planes.astype(np.float64) - p64).max())
    lsb = int(np.abs(faces.astype(int) - f64.astype(int)).max())
    print(f"{what} {case}: e32 {e32:.3e}  max|GPU - M64| {err:.3e}  bound {bound:.3e}  u8 {lsb} LSB")
    assert err <= bound, (what, case, err, bound)
    assert lsb <= 1, (what, case, lsb)


def _stack(ts):
    return np.stack([t.cpu().numpy() for t in ts])


def test_block_shape_of_the_source():
    src = open(os.path.join(ROOT, "fast-artistic-videos_amd", "csrc", "kernels_equi.hip")).read()
    assert f"dim3({BLOCK_W}, {BLOCK_H})" in src and f"(wplus + {BLOCK_W - 1}) / {BLOCK_W}, (hplus + {BLOCK_H - 1}) / {BLOCK_H}, 6" in src
    assert CASES[-1][2] % BLOCK_W == 1 and CASES[-1][2] % BLOCK_H == 1 and CASES[-1][2] > BLOCK_W


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-e%d-o%d-s%d" % c)
def test_kernel_against_the_model(favlib, cuda, case):
    ew, eh, edge, ov, ss = case
    img = _model(case)[0]
    faces, planes = favlib.vr_equi_to_faces(_dev(img, cuda), edge, ov, supersample=ss, want_f32=True)
    _gate(case, _stack(faces), _stack(planes), "kernel")


def test_outputs_do_not_depend_on_what_they_held_and_streams_agree(favlib, cuda):
    """the smallest case into NaN / 0x7f poisoned outputs; a second call on another stream gives the same bits"""
    import ctypes as C
    import torch
    case = CASES[0]
    ew, eh, edge, ov, ss = case
    src = _dev(_model(case)[0], cuda)
    first_u8, first_f32 = favlib.vr_equi_to_faces(src, edge, ov, supersample=ss, want_f32=True)
    torch.cuda.synchronize()
    u8 = [torch.full((edge, edge, 3), 0x7F, dtype=torch.uint8, device=cuda) for _ in range(6)]
    f32 = [torch.full((edge, edge, 3), float("nan"), dtype=torch.float32, device=cuda) for _ in range(6)]
    arr = lambda ts: (C.c_void_p * 6)(*[t.data_ptr() for t in ts])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rc = favlib.lib().fav_vr_equi_to_faces_rgb8(C.c_void_p(src.data_ptr()), ew, eh, edge, edge, ov, ov, ss, arr(u8), arr(f32), C.c_void_p(side.cuda_stream))
    assert rc == 0, favlib.lib().fav_last_error()
    side.synchronize()
    _gate(case, _stack(u8), _stack(f32), "poisoned outputs")
    for k in range(6):
        assert torch.equal(u8[k], first_u8[k]) and torch.equal(f32[k], first_f32[k]), k


def test_round_trip_on_the_device(favlib, cuda):
    """the kernel's u8 faces, composed into the strip and sampled through fav_vr_map_host(kind 4) on the host, give the source image back
    to within the CPU test's gate sqrt(e_ok e_bad)"""
    p = E.round_trip_premise(favlib.vr_map_host)
    c = E.RT
    faces = favlib.vr_equi_to_faces(_dev(p["image"], cuda), c["edge"], c["overlap"], supersample=c["supersample"])
    err = E.round_trip_error(list(_stack(faces)), p["map"], p["image"])
    print(f"round trip of the kernel's faces: {err:.4f}  (model {p['e_ok']:.4f}, smallest wrong variant {p['e_bad']:.4f}, gate {p['gate']:.4f})")
    assert p["e_bad"] >= 10 * p["e_ok"]
    assert err < p["gate"]


# ------------------------------------------------------------------------------------------------ the executables
EDGE, OV, EW, EH, NFR = 64, 24, 160, 80, 3      # faces and overlap of test_gpu_cli.py's smallest VR test


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (cmd, r.stdout[-2000:], r.stderr[-2000:])
    return r


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """three equirectangular frames of the sphere function, turned by 0.02 rad per frame, and route A's files: fav_transform_vr's faces and
    the two flows of every face and frame from fav_flow -batch"""
    d = tmp_path_factory.mktemp("equi_clip")
    frames = [E.sphere_image(EW, EH, 0.02 * n) for n in range(NFR)]
    for n, f in enumerate(frames):
        E.write_ppm(str(d / f"frame_{n + 1:05d}.ppm"), f)
    _run([os.path.join(BIN, "fav_transform_vr"), "-input_equi_pattern", str(d / "frame_%05d.ppm"), "-output_pattern", str(d / "faces" / "frame_%05d-%d.ppm"),
          "-cube_edge_length", str(EDGE), "-overlap_pixel_w", str(OV), "-overlap_pixel_h", str(OV)])
    lines = []
    for face in E.PROC_ORDER:
        os.makedirs(d / f"flow-{face}")
        for fr in range(2, NFR + 1):
            cur, prev = d / "faces" / f"frame_{fr:05d}-{face}.ppm", d / "faces" / f"frame_{fr - 1:05d}-{face}.ppm"
            lines += [f"{cur} {prev} {d}/flow-{face}/backward_{fr}_{fr - 1}.flo", f"{prev} {cur} {d}/flow-{face}/forward_{fr - 1}_{fr}.flo"]
    (d / "list.txt").write_text("\n".join(lines) + "\n")
    _run([os.path.join(BIN, "fav_flow"), "-batch", str(d / "list.txt")])
    return d, frames


def test_fav_transform_vr_equals_the_library(favlib, cuda, clip):
    d, frames = clip
    assert sorted(os.listdir(d / "faces")) == sorted(f"frame_{fr:05d}-{face}.ppm" for fr in range(1, NFR + 1) for face in range(1, 7))   # stops at the first missing frame
    for n, f in enumerate(frames):
        faces = favlib.vr_equi_to_faces(_dev(f, cuda), EDGE, OV)
        for k, face in enumerate(E.PROC_ORDER):
            got = favlib.read_pnm(str(d / "faces" / f"frame_{n + 1:05d}-{face}.ppm"))
            assert got.shape == (EDGE, EDGE, 3) and np.array_equal(got, faces[k].cpu().numpy()), (n, face)
    # the frames move: the flows route A reads are not zero
    assert np.abs(favlib.read_flo(str(d / "flow-1" / "backward_2_1.flo"))).max() > 0.05


@pytest.mark.parametrize("mode", ["structure0", "structure1", "inconsistent"])
def test_the_two_routes_agree(favlib, clip, tmp_path, mode):
    """route A: faces and flows from files (fav_transform_vr, fav_flow, fav_stylize_vr -input_pattern -flow_pattern -forward_flow_pattern);
    route B: fav_stylize_vr -input_equi_pattern.  The batch's flows are bit-identical to single estimates: the PNG files are byte-equal."""
    d, _ = clip
    common = ["-model_vid", VID, "-model_img", "self", "-gpu", "0", "-overlap_pixel_w", str(OV), "-overlap_pixel_h", str(OV), "-out_equi", "-out_equi_w", "96",
              "-out_equi_h", "48", "-out_cubemap", "-poll_settle", "0", "-poll_timeout", "20"]
    common += ["-create_inconsistent"] if mode == "inconsistent" else ["-structure", mode[-1]]
    files = ["-input_pattern", str(d / "faces" / "frame_%05d-%d.ppm")]
    if mode != "inconsistent":
        files += ["-flow_pattern", str(d / "flow-%d" / "backward_[%d]_{%d}.flo"), "-forward_flow_pattern", str(d / "flow-%d" / "forward_{%d}_[%d].flo")]
    exe = os.path.join(BIN, "fav_stylize_vr")
    _run([exe] + files + common + ["-output_prefix", str(tmp_path / "a" / "out")])
    _run([exe, "-input_equi_pattern", str(d / "frame_%05d.ppm"), "-cube_edge_length", str(EDGE)] + common + ["-output_prefix", str(tmp_path / "b" / "out")])
    names = sorted(f"out-{fr:05d}_{kind}.png" for fr in range(1, NFR + 1) for kind in ("equi", "cubemap"))
    assert sorted(os.listdir(tmp_path / "a")) == names and sorted(os.listdir(tmp_path / "b")) == names      # nothing else on disk
    for nm in names:
        a, b = (open(tmp_path / k / nm, "rb").read() for k in ("a", "b"))
        assert len(a) > 100 and a == b, nm
    # the frames differ, and frames 2.. depend on the flows: the comparison is not one of three equal pictures
    assert open(tmp_path / "b" / names[0], "rb").read() != open(tmp_path / "b" / names[2], "rb").read()
