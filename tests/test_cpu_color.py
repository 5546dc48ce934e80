"""-original_colors without a GPU: the properties of the numpy model of the luminance transfer (tests/util/color_model.py) that the GPU
suite then holds the kernels to -- identity, grey originals, the luminance that arrives, fp32 against fp64 -- and what fav_stylize
refuses before it opens a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import color_model as CM  # noqa: E402
import yuv_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLIZE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
MATRICES = ["601", "709"]
N = 400


@pytest.fixture(scope="module")
def images():
    """400 x 400 uniform-random bytes: the stylised frame's bytes S and the original's O"""
    rng = np.random.default_rng(20)
    return rng.integers(0, 256, (N, N, 3), dtype=np.uint8), rng.integers(0, 256, (N, N, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("matrix", MATRICES)
def test_identity_a_frame_transferred_onto_itself_is_itself(images, matrix):
    for a in images:
        for dt in (np.float32, np.float64):
            assert np.array_equal(CM.transfer_bytes(a, a, matrix, dt), a)


@pytest.mark.parametrize("matrix", MATRICES)
def test_grey_original_gives_grey_with_the_stylised_luminance(images, matrix):
    S, O = images
    grey = np.repeat(O[..., :1], 3, axis=2)
    ys = CM.luma(S, matrix, np.float64)
    for dt in (np.float32, np.float64):
        P = CM.transfer_bytes(S, grey, matrix, dt)
        assert np.array_equal(P[..., 0], P[..., 1]) and np.array_equal(P[..., 1], P[..., 2])
        assert np.abs(P[..., 0].astype(np.float64) - np.round(ys)).max() <= 1


@pytest.mark.parametrize("matrix", MATRICES)
def test_luminance_of_the_result_is_the_stylised_luminance_where_nothing_clamps(images, matrix):
    """three roundings of at most 0.5, weighted by coefficients that sum to 1: |luma(P) - ys| <= 0.5"""
    S, O = images
    raw = CM.transfer_unquantised(S, O, matrix, np.float64)
    free = ((np.floor(raw + 0.5) >= 0) & (np.floor(raw + 0.5) <= 255)).all(axis=2)
    share = free.mean()
    print(f"BT.{matrix}: {100 * share:.1f} % of the pixels do not clamp")
    assert share >= 0.5, "the check has (nearly) nothing to look at"
    P = CM.transfer_bytes(S, O, matrix, np.float64)
    err = np.abs(CM.luma(P, matrix, np.float64) - CM.luma(S, matrix, np.float64))[free]
    print(f"BT.{matrix}: largest luminance error {err.max():.6f}")
    assert err.max() <= 0.5 + 1e-9


@pytest.mark.parametrize("matrix", MATRICES)
def test_fp32_model_is_the_fp64_model_up_to_rare_ties(images, matrix):
    S, O = images
    a = CM.transfer_bytes(S, O, matrix, np.float32).astype(np.int32)
    b = CM.transfer_bytes(S, O, matrix, np.float64).astype(np.int32)
    diff = np.abs(a - b)
    print(f"BT.{matrix}: {100 * (diff != 0).mean():.4f} % of the bytes differ, by at most {diff.max()}")
    assert diff.max() <= 1 and (diff != 0).mean() <= 1e-3


def test_planes_are_the_conversion_of_the_images_bytes():
    """the model's Y4M route IS yuv_model.rgb_to_yuv of P, for a state with values outside [0, 1]"""
    rng = np.random.default_rng(21)
    state = rng.uniform(-0.3, 1.3, (3, 9, 17)).astype(np.float32)
    O = rng.integers(0, 256, (9, 17, 3), dtype=np.uint8)
    for f in M.ALL_FORMATS:
        P = CM.transfer(state, O, f.matrix)
        assert np.array_equal(P, CM.transfer_bytes(M.quantise_f32_image(state), O, f.matrix))
        assert np.array_equal(CM.transfer_yuv(state, O, f), M.rgb_to_yuv(P, f))


# ------------------------------------------------------------------------------------------------ 2. the CLI refuses before the device
@pytest.mark.parametrize("args,msgs", [
    (["-original_colors", "2"], ["-original_colors must be 0 or 1"]),
    (["-original_colors", "yes"], ["-original_colors must be 0 or 1"]),
    (["-original_colors", "1", "-continue_with", "5"], ["-original_colors 1", "-continue_with 5"]),
], ids=["value-2", "value-yes", "continue-with"])
def test_fav_stylize_refuses_before_the_device(tmp_path, args, msgs):
    assert os.path.exists(STYLIZE), "fav_stylize is not built"
    r = subprocess.run([STYLIZE, "-input_pattern", "f_%05d.ppm", "-estimate_flow", "1"] + args, capture_output=True, text=True, timeout=60,
                       stdin=subprocess.DEVNULL, cwd=tmp_path)
    assert r.returncode != 0, r.stderr
    for m in msgs:
        assert m in r.stderr, r.stderr
    assert "unknown option" not in r.stderr and "HIP" not in r.stderr and r.stdout == ""
    assert os.listdir(tmp_path) == [], "a refused run left files behind"


def test_abi_and_binding_carry_the_entry_points(favlib):
    hdr = open(os.path.join(ROOT, "include", "fav.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("fav_color_transfer_rgb8", "fav_color_transfer_yuv", "fav_stream_encode_png_colors", "fav_stream_encode_yuv_colors"):
        assert name in favlib.EXPORTS and hasattr(favlib.lib(), name) and name + "(" in hdr and name in integration, name
    assert callable(favlib.color_transfer)
