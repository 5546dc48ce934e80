"""Host side of the estimator's median filter (fav_flow_opts_ex3.median; no GPU needed): the model's median against a brute-force sort, the
ABI of the _ex3 entries, the flags of the three executables, the resource report of the new kernel next to the old ones, and the premise
-- what the filter gains on the scenes the other options were measured on -- with the fp64 models."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402
import flow_robust_model as R  # noqa: E402
import flow_match_model as P  # noqa: E402
import flow_median_model as D  # noqa: E402
from flow_testing import kernel_resource_usage  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fast-artistic-videos_amd")
BIN = os.path.join(PKG, "bin")
FLOW, STYLIZE, STYLIZE_VR = (os.path.join(BIN, n) for n in ("fav_flow", "fav_stylize", "fav_stylize_vr"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=60)


# ------------------------------------------------------------------------------------------------ 1. the model's median
def _brute(f, size):
    """every pixel's window gathered with Python loops and sorted with sorted(): shares nothing with the model but the definition"""
    h, w, c = f.shape
    r = size // 2
    out = np.empty_like(f)
    for y in range(h):
        for x in range(w):
            for k in range(c):
                win = [f[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1), k] for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
                out[y, x, k] = sorted(win)[len(win) // 2]
    return out


def _ramp(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([0.25 * xs + 0.5 * ys, 1.0 - 0.125 * xs + 0.75 * ys], -1).astype(np.float32)


@pytest.mark.parametrize("size", [3, 5])
def test_model_median_is_the_sorted_windows_middle(size):
    h, w = 17, 19
    f = _ramp(h, w)
    for y, x, v in ((8, 9, 100.0), (8, 10, -80.0), (0, 7, 50.0), (16, 3, -60.0), (5, 0, 70.0), (0, 0, 90.0), (16, 18, -90.0), (3, 15, 40.0), (4, 15, 41.0)):
        f[y, x] += np.float32(v)          # isolated spikes in the interior, on every kind of edge and in two corners; one pair of neighbours
    got = D.median(f, size)
    assert got.dtype == np.float32 and np.array_equal(got, _brute(f, size))
    assert not np.array_equal(got, f)
    const = np.full((h, w, 2), np.float32(-2.5))
    assert np.array_equal(D.median(const, size), const)
    # a ramp along one axis (u along x, v along y: every value of a window occurs 2r + 1 times) is its own median, and one interior
    # spike goes
    ys, xs = np.mgrid[0:h, 0:w]
    ramp = np.stack([0.25 * xs, 1.0 + 0.75 * ys], -1).astype(np.float32)
    spiked = ramp.copy(); spiked[8, 9] += np.float32(1000.0)
    assert np.array_equal(D.median(spiked, size), D.median(ramp, size))
    r = size // 2
    assert np.array_equal(D.median(spiked, size)[r:-r, r:-r], ramp[r:-r, r:-r])
    # the filter off is the model of the other options, bit for bit
    if size == 3:
        A, B = M.warped_pair(32, 40, 11)
        assert np.array_equal(D.flow(A, B), M.flow(A, B)) and np.array_equal(D.flow(A, B, eps=R.EPS), R.flow(A, B))
        assert np.array_equal(D.flow(A, B, beta=P.BETA, grad=True), P.flow(A, B, grad=True))


# ------------------------------------------------------------------------------------------------ 2. the ABI
EX3_ENTRIES = ("fav_flow_workspace_bytes_ex3", "fav_flow_rgb8_ex3", "fav_flow_pairs_workspace_bytes_ex3", "fav_flow_pairs_rgb8_ex3",
               "fav_stream_next_frame_estimate_ex3", "fav_flow_median_f32")


def test_ex3_entries_struct_sizes_and_workspace(favlib):
    L = favlib.lib()
    assert C.sizeof(favlib._FlowOptsEx3) == C.sizeof(favlib._FlowOptsEx2) + 4 == 40
    hdr = open(os.path.join(ROOT, "include", "fav.h")).read()
    assert "typedef struct fav_flow_opts_ex3 { fav_flow_opts_ex2 ex2; int median; } fav_flow_opts_ex3;" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", favlib.LIB_PATH], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EX3_ENTRIES:
        assert name in defined and name in favlib.EXPORTS and name + "(" in hdr and name in integration, name
    assert callable(favlib.flow_median)
    void = lambda o: C.cast(C.pointer(o), C.c_void_p)
    for (w, h) in ((1280, 720), (64, 64), (150, 203)):
        for opts in ({}, dict(smooth_eps=0.3), dict(match_beta=-1), dict(match_beta=-1, smooth_eps=0.3), dict(data_term=1)):
            old = L.fav_flow_workspace_bytes_ex2(w, h, void(favlib._flow_opts_ex2(opts)))
            assert old > 0
            for median in (0, 3, 5):
                o = favlib._flow_opts_ex3(dict(opts, median=median))
                assert o.median == median
                assert L.fav_flow_workspace_bytes_ex3(w, h, void(o)) == old == favlib.flow_workspace_bytes(w, h, median=median, **opts), (w, h, opts, median)
                for n in (1, 6):
                    assert L.fav_flow_pairs_workspace_bytes_ex3(w, h, n, void(o)) == L.fav_flow_pairs_workspace_bytes_ex2(w, h, n, void(favlib._flow_opts_ex2(opts))) > 0
        assert L.fav_flow_workspace_bytes_ex3(w, h, None) == L.fav_flow_workspace_bytes_ex2(w, h, None) > 0


def test_bad_median_options_are_refused_before_the_device(favlib):
    L = favlib.lib()
    void = lambda o: C.cast(C.pointer(o), C.c_void_p)
    one = (C.c_void_p * 1)(256)
    p, q = C.c_void_p(256), C.c_void_p(1 << 20)
    for median in (1, 2, 4, 7, -1):
        o = favlib._flow_opts_ex3(dict(median=median))
        msg = b"median must be 0 (off), 3 or 5"
        named = b"not %d" % median
        assert L.fav_flow_workspace_bytes_ex3(64, 64, void(o)) == 0 and msg in L.fav_last_error() and named in L.fav_last_error(), median
        assert L.fav_flow_pairs_workspace_bytes_ex3(64, 64, 2, void(o)) == 0 and named in L.fav_last_error(), median
        assert L.fav_flow_rgb8_ex3(p, p, 64, 64, C.byref(o), p, p, C.c_size_t(1 << 30), None) == -1 and named in L.fav_last_error(), median      # FAV_EINVAL
        assert L.fav_flow_pairs_rgb8_ex3(one, one, 1, 64, 64, C.byref(o), one, one, p, C.c_size_t(1 << 30), None) == -1 and named in L.fav_last_error(), median
        with pytest.raises(favlib.FavError, match="median must be"):
            favlib.flow_workspace_bytes(64, 64, median=median)
    # the other options are still checked through the _ex3 entries
    assert L.fav_flow_workspace_bytes_ex3(64, 64, void(favlib._flow_opts_ex3(dict(median=5, data_term=2)))) == 0 and b"data_term must be" in L.fav_last_error()
    assert L.fav_flow_workspace_bytes_ex3(64, 64, void(favlib._flow_opts_ex3(dict(median=5, match_radius=40)))) == 0 and b"match_radius must be" in L.fav_last_error()
    with pytest.raises(favlib.FavError, match="unknown flow option"):
        favlib.flow_workspace_bytes(64, 64, medians=5)
    # the stage entry's own checks: the size, and buffers that overlap (64 x 64 x 8 = 32768 bytes each)
    for size in (0, 1, 4, 7, -3):
        assert L.fav_flow_median_f32(p, q, 64, 64, size, None) == -1 and b"size must be 3 or 5" in L.fav_last_error() and b"not %d" % size in L.fav_last_error(), size
    for a, b in ((256, 256), (256, 256 + 32768 - 8), (256 + 32768 - 8, 256), (1024, 512)):
        assert L.fav_flow_median_f32(C.c_void_p(a), C.c_void_p(b), 64, 64, 5, None) == -1 and b"overlap" in L.fav_last_error(), (a, b)
    assert L.fav_flow_median_f32(None, q, 64, 64, 5, None) == -1 and L.fav_flow_median_f32(p, None, 64, 64, 5, None) == -1
    assert L.fav_flow_median_f32(p, q, 0, 64, 5, None) == -1
    assert L.fav_flow_median_f32(C.c_void_p(260), q, 64, 64, 5, None) == -1 and b"8-byte aligned" in L.fav_last_error()
    import torch
    if not torch.cuda.is_available():      # valid arguments, no device: FAV_ENODEVICE before anything is dereferenced
        assert L.fav_flow_median_f32(p, C.c_void_p(256 + 32768), 64, 64, 5, None) == -6
        o = favlib._flow_opts_ex3(dict(median=5))
        nb = favlib.flow_workspace_bytes(64, 64, median=5)
        assert L.fav_flow_rgb8_ex3(p, p, 64, 64, C.byref(o), p, p, C.c_size_t(nb), None) == -6
        assert L.fav_flow_rgb8_ex3(p, p, 64, 64, C.byref(o), p, p, C.c_size_t(nb - 1), None) == -1


# ------------------------------------------------------------------------------------------------ 3. the flags
def test_fav_flow_median_flag(favlib, tmp_path):
    r = _run([FLOW])
    assert r.returncode == 2 and "[-median 0|3|5]" in r.stderr
    for bad in ("4", "1", "7", "-1", "yes"):
        r = _run([FLOW, "-median", bad, "a.ppm", "b.ppm", "c.flo"])
        assert r.returncode != 0 and "-median must be 0, 3 or 5" in r.stderr, (bad, r.stderr)
    for ok in ("0", "3", "5"):
        r = _run([FLOW, "-median", ok, "-match", "1", "-grad", "1", "-eps", "0.3", str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm"), str(tmp_path / "c.flo")])
        assert r.returncode == 1 and "usage" not in r.stderr and ("no HIP device" in r.stderr or "Could not open" in r.stderr), r.stderr      # accepted


def test_fav_stylize_flow_median_flag(favlib):
    base = [STYLIZE, "-input_pattern", "v/f_%05d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/out"]
    for ok in ("0", "3", "5"):
        r = _run(base + ["-estimate_flow", "1", "-flow_median", ok, "-flow_match", "1", "-flow_grad", "1", "-flow_eps", "0.3", "-dry_run", "1"])
        assert r.returncode == 0, r.stderr
    r = _run(base + ["-flow_pattern", "v/b_%05d.flo", "-occlusions_pattern", "v/r_%05d.pgm", "-flow_median", "5", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_median" in r.stderr and "-estimate_flow 1" in r.stderr, r.stderr
    r = _run(base + ["-flow_pattern", "v/b_%05d.flo", "-occlusions_pattern", "v/r_%05d.pgm", "-flow_median", "0", "-dry_run", "1"])
    assert "-flow_median" not in r.stderr, r.stderr
    for bad in ("4", "1", "-1"):
        r = _run(base + ["-estimate_flow", "1", "-flow_median", bad, "-dry_run", "1"])
        assert r.returncode != 0 and "-flow_median must be 0, 3 or 5" in r.stderr, r.stderr


def test_fav_stylize_vr_flow_median_flag(favlib):
    equi = [STYLIZE_VR, "-input_equi_pattern", "v/e_%05d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/out"]
    ok = _run(equi + ["-dry_run", "1"])
    r = _run(equi + ["-flow_median", "5", "-flow_match", "1", "-flow_grad", "1", "-flow_eps", "0.3", "-dry_run", "1"])
    assert r.returncode == ok.returncode and "unknown option" not in r.stderr and "-flow_median" not in r.stderr, r.stderr
    faces = [STYLIZE_VR, "-input_pattern", "v/f_%05d-%d.ppm", "-flow_pattern", "v/b_%05d-%d.flo", "-occlusions_pattern", "v/r_%05d-%d.pgm", "-model_vid", "m.t7",
             "-output_prefix", "o/out"]
    r = _run(faces + ["-flow_median", "5", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_median" in r.stderr and "-input_equi_pattern" in r.stderr, r.stderr
    r = _run(equi + ["-flow_median", "4", "-dry_run", "1"])
    assert r.returncode != 0 and "-flow_median must be 0, 3 or 5" in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ 4. the resource gate
def _design_rows():
    """{kernel name as DESIGN.md writes it: (lanes, VGPRs, AGPRs, scratch, LDS bytes, occupancy)} of its resource tables"""
    rows = {}
    for line in open(os.path.join(ROOT, "DESIGN.md")):
        m = re.match(r"\| `(flow_\w+(?:<[^>]*>)?)` \|((?: [\d ]+ \|){6})\s*$", line)
        if m:
            rows[m.group(1)] = tuple(int(c.replace(" ", "")) for c in m.group(2).strip(" |").split("|"))
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_median_kernels_stay_in_registers_and_the_old_kernels_keep_their_figures(tmp_path):
    """the compiler's kernel-resource-usage remarks for kernels_flow.hip (flow_testing.kernel_resource_usage).  flow_median_kernel keeps its
    9 | 25 window values in registers through a selection network whose indices are constants: scratch 0, AGPRs 0 (measured: 24 | 62
    VGPRs, 9 504 | 10 880 B of LDS, occupancy 8).  The filter adds a kernel and touches none: the four sweep and the four coefficient
    instantiations report what DESIGN.md's table says."""
    usage = kernel_resource_usage(HIPCC, tmp_path)
    rows = _design_rows()
    median = {k: u for k, u in usage.items() if "flow_median_kernel" in k}
    assert sorted(k[k.index("flow_median_kernel"):][:24] for k in median) == ["flow_median_kernelILi1EE", "flow_median_kernelILi2EE"], sorted(usage)
    for k, u in median.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0 and u["Occupancy"] >= 2 and 0 < u["LDS"] <= 16384, (k, u)
        row = rows["flow_median_kernel<1>" if "ILi1E" in k else "flow_median_kernel<2>"]
        assert row == (256, u["VGPRs"], 0, 0, u["LDS"], u["Occupancy"]), (k, u, row)
    old = {"flow_sweep_kernel<BrightCell, false>": "flow_sweep_kernelINS0_10BrightCellELb0EEE", "flow_sweep_kernel<BrightCell, true>": "flow_sweep_kernelINS0_10BrightCellELb1EEE",
           "flow_sweep_kernel<GradCell, false>": "flow_sweep_kernelINS0_8GradCellELb0EEE", "flow_sweep_kernel<GradCell, true>": "flow_sweep_kernelINS0_8GradCellELb1EEE",
           "flow_coef_kernel<false>": "flow_coef_kernelILb0EEE", "flow_coef_kernel<true>": "flow_coef_kernelILb1EEE",
           "flow_coef_grad_kernel<false>": "flow_coef_grad_kernelILb0EEE", "flow_coef_grad_kernel<true>": "flow_coef_grad_kernelILb1EEE"}
    assert len([k for k in usage if "flow_sweep_kernel" in k]) == 4
    for name, mangled in old.items():
        hit = [u for k, u in usage.items() if mangled in k]
        assert len(hit) == 1, (name, sorted(usage))
        u = hit[0]
        assert rows[name][1:] == (u["VGPRs"], u["AGPRs"], u["ScratchSize"], u["LDS"], u["Occupancy"]), (name, u, rows[name])


# ------------------------------------------------------------------------------------------------ 5. the premise
# fp64 models, mean endpoint error in px, as measured when the option was built; the test holds every figure to 10 % against drift of the
# models and states what the filter does to it.  (median off, 3, 5)
TWO_MOTION = {(1, 0.0): (0.9971, 0.9829, 0.9522), (1, R.EPS): (0.6280, 0.6206, 0.5949),
              (2, 0.0): (1.1442, 1.1375, 1.1126), (2, R.EPS): (0.7271, 0.7331, 0.7151)}
HALF_OBJECT = (4.3516, 4.3228, 4.1563)
DRIFT = 0.10


@pytest.mark.parametrize("seed,eps", sorted(TWO_MOTION))
def test_premise_two_motion_scene(seed, eps):
    """flow_robust_model.two_motion_scene(96, 128, seed): non-occluded pixels, 12 px of frame border excluded; the quadratic term (alpha 15)
    and eps 0.3 (alpha 5).  Measured, off -> 3 x 3 -> 5 x 5:
      seed 1: 0.9971 -> 0.9829 -> 0.9522 px;  with eps 0.3: 0.6280 -> 0.6206 -> 0.5949 px
      seed 2: 1.1442 -> 1.1375 -> 1.1126 px;  with eps 0.3: 0.7271 -> 0.7331 -> 0.7151 px
    The 5 x 5 filter lowers the error on every scene, by 2 .. 5 %; the 3 x 3 filter by about 1 % and, on seed 2 with eps 0.3, not at all
    (+0.8 %).  Required: each figure within 10 % of the measured one, and 5 x 5 below off."""
    A, B, truth, valid = R.two_motion_scene(96, 128, seed)
    got = tuple(R.scene_epe(D.flow(A, B, eps=eps, median_size=m, dtype=np.float64), truth, valid) for m in (0, 3, 5))
    print(f"two-motion scene seed {seed} eps {eps}: off {got[0]:.4f}  3x3 {got[1]:.4f}  5x5 {got[2]:.4f} px")
    for g, want in zip(got, TWO_MOTION[(seed, eps)]):
        assert abs(g - want) <= DRIFT * want, (got, TWO_MOTION[(seed, eps)])
    assert got[2] < got[0]


def test_premise_object_with_the_matching_prior():
    """flow_match_model.half_scene() (96 x 128, a 20 x 20 object moving (11, -7) over a background moving (1, 0)), the prior on (beta 225,
    R 8): error on the object.  Measured, off -> 3 x 3 -> 5 x 5: 4.3516 -> 4.3228 -> 4.1563 px (background 0.8623 -> 0.8608 -> 0.8656):
    the filter takes 4.5 % off what the prior leaves, it does not repair a wrong match.  Required: within 10 % of the measured figures,
    and 5 x 5 below off."""
    A, B, truth, valid, obj = P.half_scene()
    got = tuple(P.scene_errors(D.flow(A, B, beta=P.BETA, radius=8, median_size=m, dtype=np.float64), truth, valid, obj)[0] for m in (0, 3, 5))
    print(f"half scene with the prior, object: off {got[0]:.4f}  3x3 {got[1]:.4f}  5x5 {got[2]:.4f} px")
    for g, want in zip(got, HALF_OBJECT):
        assert abs(g - want) <= DRIFT * want, (got, HALF_OBJECT)
    assert got[2] < got[0]


@pytest.mark.parametrize("seed", [1, 2])
def test_premise_pure_translation_costs_nothing(seed):
    """flow_model.shifted_pair (a constant flow of (3.5, -2.25) px): the existing premise bound of 0.5 px holds with the 5 x 5 filter.
    Measured, off -> 3 x 3 -> 5 x 5: seed 1 0.0656 -> 0.0635 -> 0.0559 px, seed 2 0.0984 -> 0.0952 -> 0.0860 px."""
    A, B, t = M.shifted_pair(seed)
    got = tuple(M.interior_epe(D.flow(A, B, median_size=m, dtype=np.float64), t) for m in (0, 3, 5))
    print(f"shifted pair seed {seed}: off {got[0]:.4f}  3x3 {got[1]:.4f}  5x5 {got[2]:.4f} px")
    assert got[2] <= 0.5 and got[1] <= 0.5
