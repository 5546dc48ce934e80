"""360 degrees from equirectangular frames, the part that needs no GPU: the numpy model of the transform (tests/util/equi_model.py)
against the project's own cube -> equirectangular map, the flags of bin/fav_transform_vr and of fav_stylize_vr -input_equi_pattern,
the exported symbol and the binding.

Measured on the round-trip case (192 x 96 -> edge 48, overlap 8, supersample 2; grey levels, mean absolute error against the source):
e_ok 0.243; wrong variants: faces 1 and 2 swapped 15.39, face 5 not rotated 10.50, face 1 mirrored 3.98, overlap margin ignored 3.76
-> e_bad 3.76, e_bad / e_ok 15.5, gate sqrt(e_ok e_bad) 0.956.  max|M32 - M64| on that case: 6.3e-05."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import equi_model as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
VR = os.path.join(BIN, "fav_stylize_vr")
TR = os.path.join(BIN, "fav_transform_vr")
EQUI = [VR, "-input_equi_pattern", "v/f_%05d.ppm", "-model_vid", "m.t7"]


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=60)


# ------------------------------------------------------------------------------------------------ the model
def test_round_trip_premise(favlib):
    """faces of the fp64 model, composed into the strip and sampled through fav_vr_map_host(kind 4), give the source image back; each
    wrong transform (two faces swapped, face 5 not rotated, a face mirrored, the margin ignored) is at least ten times further away"""
    p = E.round_trip_premise(favlib.vr_map_host)
    print(f"e_ok {p['e_ok']:.4f}  e_bad {p['e_bad']:.4f}  ratio {p['e_bad'] / p['e_ok']:.2f}  gate {p['gate']:.4f}")
    for name, e in p["wrong"].items():
        print(f"  {name}: {e:.4f}")
    assert len(p["wrong"]) == 4
    assert p["e_bad"] >= 10 * p["e_ok"], (p["e_ok"], p["wrong"])
    assert p["e_ok"] < p["gate"] < p["e_bad"]


def test_fp32_model_against_fp64_model(favlib):
    """max|M32 - M64| on the round-trip case, the figure the GPU bound rests on.  Its size by reasoning: a coordinate below 192 carries
    half an fp32 ulp, 7.6e-6 pixels, through atan2 and the product, a few times over; the image changes by at most a few grey levels per
    pixel; values up to 255 round by 1.5e-5 in each of the ~20 operations of the two cubics and the mean: 1e-3 at the very most."""
    p = E.round_trip_premise(favlib.vr_map_host)
    e32 = float(np.abs(p["planes32"].astype(np.float64) - p["planes"]).max())
    print(f"max|M32 - M64| {e32:.3e}")
    assert p["planes32"].dtype == np.float32 and p["planes"].dtype == np.float64
    assert 0 < e32 < 1e-3


def test_one_sample_of_a_constant_image_is_the_constant():
    for value in (0, 1, 77, 255):
        img = np.full((41, 97, 3), value, np.uint8)
        for dt in (np.float64, np.float32):
            faces, planes = E.equi_to_faces(img, 24, 24, 0, 0, 1, dt)
            assert (planes == value).all() and (faces == value).all(), (value, dt)


def test_a_feature_at_longitude_zero_crosses_the_seam_intact():
    """a bright bar across columns W-3 .. 3 of the frame lies in the middle of position 3's face (direction -z); the columns wrap, so the
    face shows what position 0's face shows of the same bar moved half-way round (to longitude pi)"""
    ew, eh, edge, ov = 128, 64, 32, 8
    img = np.zeros((eh, ew, 3), np.uint8)
    cols = np.arange(-3, 4) % ew
    img[20:44, cols] = (250, 180, 90)
    _, seam = E.equi_to_faces(img, edge, edge, ov, ov, 2)
    _, moved = E.equi_to_faces(np.roll(img, ew // 2, axis=1), edge, edge, ov, ov, 2)
    assert np.abs(seam[3] - moved[0]).max() < 1e-8
    # a = 0 at sx = overlap / 2 + (edge - overlap) / 2 = 16: the bar's middle, full brightness, and dark well away from it
    assert np.allclose(seam[3][16, 16], (250, 180, 90), atol=1e-6) and np.abs(seam[3][16, 15] - seam[3][16, 17]).max() < 1e-6
    assert np.abs(seam[3][16, :8]).max() < 1.0 and np.abs(seam[3][16, 25:]).max() < 1.0
    # without the wrap (the columns clamped instead) the left half of the bar would be missing: the model must not be symmetric by accident
    assert seam[3][16, 14:19, 0].min() > 100


# ------------------------------------------------------------------------------------------------ flags
def test_fav_stylize_vr_equi_mode_needs_only_its_input_and_the_model(favlib):
    r = _run(EQUI + ["-gpu", "0", "-dry_run", "1"])
    assert r.returncode == 0 and "Must give" not in r.stderr, r.stderr
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["streams"][0]["input_equi_pattern"] == "v/f_%05d.ppm" and rec["streams"][0]["input_pattern"] == ""
    r = _run(EQUI + ["-gpu", "0", "-dry_run", "1", "-cube_edge_length", "64", "-supersample", "4", "-overlap_pixel_w", "24", "-overlap_pixel_h", "24",
                     "-flow_alpha", "12.5", "-flow_warps", "2", "-flow_iters", "20", "-structure", "0", "-create_inconsistent", "-out_equi", "-out_cubemap",
                     "-median_filter", "3", "-png_encoder", "host", "-start_frame", "2", "-num_frames", "5"])
    assert r.returncode == 0, r.stderr
    r = _run([VR, "-input_equi_pattern", "v/f_%05d.ppm", "-gpu", "0", "-dry_run", "1"])
    assert r.returncode != 0 and "Must give -model_vid" in r.stderr
    # the file mode's message stands when neither input is named
    r = _run([VR, "-model_vid", "m.t7", "-gpu", "0", "-dry_run", "1"])
    assert r.returncode != 0 and "Must give -input_pattern" in r.stderr


def test_fav_stylize_vr_equi_mode_refusals(favlib):
    for flag, pat in (("-input_pattern", "v/f_%05d-%d.ppm"), ("-flow_pattern", "v/flow-%d/bw_[%d]_{%d}.flo"),
                      ("-forward_flow_pattern", "v/flow-%d/fw_{%d}_[%d].flo"), ("-occlusions_pattern", "v/flow-%d/r_[%d]_{%d}.pgm")):
        r = _run(EQUI + [flag, pat, "-gpu", "0", "-dry_run", "1"])
        assert r.returncode != 0 and "-input_equi_pattern" in r.stderr and f"cannot be combined with {flag}" in r.stderr, (flag, r.stderr)
    for bad in ("0", "5", "-1", "x"):
        r = _run(EQUI + ["-supersample", bad, "-gpu", "0", "-dry_run", "1"])
        assert r.returncode != 0 and "-supersample must be 1 .. 4" in r.stderr, (bad, r.stderr)
    for bad in ("15", "0", "-64"):
        r = _run(EQUI + ["-cube_edge_length", bad, "-gpu", "0", "-dry_run", "1"])
        assert r.returncode != 0 and "-cube_edge_length must be" in r.stderr, (bad, r.stderr)
    r = _run(EQUI + ["-flow_iters", "5000", "-gpu", "0", "-dry_run", "1"])
    assert r.returncode != 0 and "iters must be" in r.stderr
    r = _run(EQUI + ["-dry_run", "1"])                                        # -gpu defaults to -1, as in the reference
    assert r.returncode != 0 and "no CPU backend" in r.stderr
    for still, msg in ((["-backward"], "-backward is not provided"), (["-smooth_certainty"], "-smooth_certainty is not provided"),
                       (["-continue_with", "2"], "-continue_with > 1"), (["-gpus", "2"], "runs on one GPU"),
                       (["-estimate_flow", "1"], "unknown option -estimate_flow")):
        r = _run(EQUI + still + ["-gpu", "0", "-dry_run", "1"])
        assert r.returncode != 0 and msg in r.stderr, (still, r.stderr)


def test_fav_transform_vr_flags(favlib):
    base = [TR, "-input_equi_pattern", "v/f_%05d.ppm", "-output_pattern", "o/f_%05d-%d.ppm"]
    r = _run(base + ["-dry_run", "1"])
    assert r.returncode == 0, r.stderr
    rec = json.loads(r.stdout.splitlines()[-1])
    assert rec == {"input_equi_pattern": "v/f_%05d.ppm", "output_pattern": "o/f_%05d-%d.ppm", "cube_edge_length": 768, "overlap_pixel_w": 128,
                   "overlap_pixel_h": 128, "supersample": 2, "start_frame": 1, "num_frames": 9999, "gpu": 0}
    r = _run([TR, "-output_pattern", "o/f_%05d-%d.ppm", "-dry_run", "1"])
    assert r.returncode != 0 and "Must give -input_equi_pattern" in r.stderr
    r = _run([TR, "-input_equi_pattern", "v/f_%05d.ppm", "-dry_run", "1"])
    assert r.returncode != 0 and "Must give -output_pattern" in r.stderr
    for flag, bad, msg in (("-supersample", "0", "-supersample must be 1 .. 4"), ("-supersample", "5", "-supersample must be 1 .. 4"),
                           ("-cube_edge_length", "15", "-cube_edge_length must be"), ("-gpu", "-1", "no CPU backend"),
                           ("-overlap_pixel_w", "768", "-overlap_pixel_w / -overlap_pixel_h must be"), ("-num_frames", "many", "bad value for -num_frames"),
                           ("-estimate_flow", "1", "unknown option -estimate_flow")):
        r = _run(base + [flag, bad, "-dry_run", "1"])
        assert r.returncode != 0 and msg in r.stderr, (flag, bad, r.stderr)


# ------------------------------------------------------------------------------------------------ symbol and binding
def test_symbol_header_binding_and_argument_checks(favlib):
    name = "fav_vr_equi_to_faces_rgb8"
    assert name in open(os.path.join(ROOT, "include", "fav.h")).read()
    for lib in (favlib.LIB_PATH, favlib.DIAG_LIB_PATH):                       # exported from both libraries
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        assert name in {l.split()[-1] for l in out.splitlines() if l.strip()}, lib
    assert name in favlib.EXPORTS and callable(favlib.vr_equi_to_faces)
    L = favlib.lib()
    p = C.c_void_p(256)
    six = (C.c_void_p * 6)(*[256] * 6)
    call = lambda *a: L.fav_vr_equi_to_faces_rgb8(*a)
    assert call(None, 192, 96, 48, 48, 8, 8, 2, six, None, None) == -1 and b"null pointer" in L.fav_last_error()
    assert call(p, 192, 96, 48, 48, 8, 8, 2, None, None, None) == -1 and b"null pointer" in L.fav_last_error()
    for s in (0, 5, -1):
        assert call(p, 192, 96, 48, 48, 8, 8, s, six, None, None) == -1 and b"supersample must be 1 .. 4" in L.fav_last_error()
    assert call(p, 192, 96, 48, 48, 48, 8, 2, six, None, None) == -1 and b"does not fit" in L.fav_last_error()
    assert call(p, 192, 96, 0, 48, 0, 0, 2, six, None, None) == -1 and b"bad face size" in L.fav_last_error()
    assert call(p, 3, 96, 48, 48, 8, 8, 2, six, None, None) == -1 and b"bad equirectangular size" in L.fav_last_error()
    hole = (C.c_void_p * 6)(256, 256, 256, None, 256, 256)
    assert call(p, 192, 96, 48, 48, 8, 8, 2, hole, None, None) == -1 and b"null face 3" in L.fav_last_error()
    import torch
    if not torch.cuda.is_available():      # valid arguments, no device: FAV_ENODEVICE before anything is dereferenced
        assert call(p, 192, 96, 48, 48, 8, 8, 2, six, None, None) == -6 and b"no CPU fallback" in L.fav_last_error()
