"""The channel regimes of tests/util/layer_probe.py (REGIMES), without a GPU: every regime probe of tests/test_gpu_stats_edges.py meets
the probe's two conditions and puts its channels where it says, the fp32 C oracle pushed through the observer stays within a quarter of
the GPU bound (at offset / sigma = 2^9, P.OFFSET_LOG2), and a numpy model of tiled InstanceNorm statistics with one planted defect at a
time is rejected by the regime that is there for it -- and accepted on the plain channels alone, which is why the regimes are there.

One claim does not hold and is asserted as what it is: a missing `var > 0` clamp cannot be seen in the flat regime.  A constant
channel of |value| <= 1 has a variance of exactly zero in the library's finalize (float64 sums of fp32 tile statistics: 0.5 and 0.25
multiply and add without rounding), and where a rounded one comes out negative it is below mean^2 x 2^-52 in magnitude -- it takes
|mean| > 3e5 to get past eps = 1e-5 inside the square root.  test_defect_c_... shows the mutant is bit for bit the model itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import layer_probe as P  # noqa: E402
from fav_amd import t7  # noqa: E402

ALL_EDGE = P.EDGE_CASES + [c for _, cs in P.EDGE_DIAG_CASES for c in cs] + P.ELEMENT_CASES
_seen = set()
ALL_EDGE = [c for c in ALL_EDGE if not (c["name"] in _seen or _seen.add(c["name"]))]


def _watched(pr):
    """float64: the tensors whose statistics L's kernels take, as [(tensor [C][H][W], regime names)]"""
    item = pr.arch.split(",")[pr.L]
    if item[0] == "U":
        tr = []
        P.forward64(pr.layers, P._t64(pr.x), tr)
        u = max(i for i, (t, _) in enumerate(tr) if t == "up")
        return [(tr[u - 1][1].numpy(), pr.regimes)]
    convs = []
    P.forward64(pr.layers, P._t64(pr.x), convs=convs)
    c0 = P.conv_index(pr.arch, pr.L)
    return [(convs[c0 + i].numpy(), pr.regimes) for i in range(2 if item[0] in "RC" else 1)]


@pytest.mark.parametrize("case", ALL_EDGE, ids=lambda c: c["name"])
def test_regime_probe_meets_the_conditions_and_reaches_its_regimes(tmp_path, case):
    pr = P.probe_for(case, "stats", tmp_path, regimes=True)
    pr.L = case["L"]
    for path in pr.paths:
        _, pre, arg = P.reference_parts(t7.extract_layers(t7.load(path)["model"]), pr.x)
        if pre is not None: assert pre.min() >= 1.0, pre.min()
        assert 0.05 <= np.abs(arg).max() <= 0.5, np.abs(arg).max()
    assert tuple(arg.shape[1:]) == tuple(case["out"])
    for g, _ in [q for p in pr.table["passes"] for q in p]:
        assert len({pr.regimes[c] for c in g}) >= min(len(g), 4)          # several regimes in every observer group
    join = case["arch"].split(",")[case["L"]][0] == "U" and "R" in case["arch"]
    for z, names in _watched(pr):
        sd, rms = P._stats(z)
        mean = z.reshape(z.shape[0], -1).mean(axis=1)
        for c, r in enumerate(names):
            if r in ("offset+", "offset-"):
                assert 2.0 ** (P.OFFSET_LOG2 - 0.6) <= abs(mean[c]) / sd[c] <= 2.0 ** (P.OFFSET_LOG2 + 0.6), (c, mean[c] / sd[c])
                assert (mean[c] > 0) == (r == "offset+")
            elif r == "big": assert 2.0 ** 10 <= rms[c] < 2.0 ** 11, (c, rms[c])
            elif r == "small":
                # (behind a norm with gamma 2^-9: sigma = 2^-9 / sqrt(1 + eps / var), a hair under 2^-9; the join: two such terms)
                lo = 2.0 ** -9 * (1 - 1e-5 if case["arch"].split(",")[case["L"]][0] == "U" else 1)
                assert lo <= sd[c] < 2.0 ** -8 * (1.5 if join else 1.0), (c, sd[c])
            elif r == "flat": assert sd[c] == 0.0 and abs(mean[c]) in (0.0, 0.5), (c, sd[c], mean[c])


@pytest.mark.parametrize("case", ALL_EDGE, ids=lambda c: c["name"])
def test_fp32_oracle_stays_within_a_quarter_of_the_bound(oracle, tmp_path, case):
    """the reference path of the GPU test is sound: plain fp32 arithmetic, pushed through the observer, meets the float64 model at no more
    than a quarter of TOL_STATS x max(1, max |ref|) under all six regimes, at offset / sigma = 2^9"""
    pr = P.probe_for(case, "stats", tmp_path, regimes=True)
    outs = [oracle.net_forward(t7.extract_layers(t7.load(path)["model"]), pr.x, []) for path in pr.paths]
    ref = P.reference_sums(pr.layers, pr.x, pr.table)
    err = P.assert_close(P.observe(outs, pr.table), ref, pr.tol, case["name"])
    print("stats edges, fp32 oracle %-24s offset/sigma 2^%d  max|ref| %7.3f  err %.2e of %.0e" % (case["name"], P.OFFSET_LOG2, np.abs(ref).max(), err, pr.tol))
    assert pr.tol == P.TOL_STATS and err <= 0.25 * pr.tol


# ------------------------------------------------------------------------------------------------ planted defects
# The library's own arrangement (kernels_*.hip epilogues, in_finalize_kernel): per tile the mean and M2 = sum (x - mean)^2 in fp32 and a
# pixel count; the finalize sums n mean and M2 + n mean^2 over the tiles in float64, divides by the TRUE pixel count, clamps the variance
# at zero and forms scale = gamma / sqrt(var + eps), shift = beta - mean scale, rounded to fp32.
TILE = (8, 32)
# One row of 63 full 8 x 32 tiles and one of 8 x 31: counting that tile as full miscounts 8 pixels of 16 376, f = 4.9e-4 of the layer.  The
# defect moves a channel's mean by ~f x mean: f x |mean| / sigma <= 5e-4 of a sigma where |mean| <~ sigma (inside the bound: the plain
# channels cannot see it), a quarter of a sigma at |mean| / sigma = 2^9.  (At 8 x 63, f = 1.6e-2, plain channels reject it as well.)
MODEL_ARCH, MODEL_HW = "c9s1-32,c3s1-64,c9s1-3", (8, 2047)


def tiled_scale_shift(z, gamma, beta, eps, defect=None):
    """z: one channel [H][W] float32 -> (scale, shift) float32.  defect: None | "a" one-pass E[x^2] - mean^2 per tile in fp32 | "b" a ragged
    tile counted as full | "c" no clamp of a negative variance | "d" eps outside the square root | "e" a unit's sum of squares saturates at 8.2e6"""
    f32 = np.float32
    s1 = s2 = 0.0
    for y0 in range(0, z.shape[0], TILE[0]):
        for x0 in range(0, z.shape[1], TILE[1]):
            v = z[y0:y0 + TILE[0], x0:x0 + TILE[1]].ravel()
            n = TILE[0] * TILE[1] if defect == "b" else v.size
            mean = f32(v.sum(dtype=f32) / f32(v.size))                      # (numpy's fp32 sums: pairwise, every partial sum rounded to fp32)
            if defect == "a": m2 = f32((v * v).sum(dtype=f32) - f32(f32(v.size) * f32(mean * mean)))
            else: d = v - mean; m2 = (d * d).sum(dtype=f32)
            sq = float(m2) + n * float(mean) ** 2
            if defect == "e": sq = min(sq, 8.2e6)
            s1 += n * float(mean); s2 += sq
    M = z.size
    mean = s1 / M
    var = s2 / M - mean * mean
    if defect != "c": var = max(var, 0.0)
    with np.errstate(invalid="ignore"):
        sc = gamma / (np.sqrt(var) + eps) if defect == "d" else gamma / np.sqrt(var + eps)
    return f32(sc), f32(beta - mean * sc)


@pytest.fixture(scope="module")
def model_parts(tmp_path_factory):
    """the regime probe of a 3 x 3 convolution in front of its norm: L's raw float64 output rounded to fp32 (what a kernel's epilogue
    holds), the observed float64 tensor, and the un-mutated model's output -- computed once, read by every test below"""
    pr = P.probe_checkpoints(MODEL_ARCH, 1, "stats", 7, MODEL_HW, tmp_path_factory.mktemp("model"), regimes=True)      # (zero-padded layers: the size stays)
    pr.tol = P.TOL_STATS
    convs = []
    P.forward64(pr.layers, P._t64(pr.x), convs=convs)
    z = convs[1].numpy().astype(np.float32)
    y = P.reference_parts(pr.layers, pr.x)[0]
    base = _model_output(pr, z, None, range(z.shape[0]), y)
    for a in (z, y, base): a.setflags(write=False)
    return pr, z, y, base


def _model_output(pr, z, defect, channels, start):
    out = np.array(start, np.float64)
    for c in channels:
        sc, sh = tiled_scale_shift(z[c], 1.0, pr.B, 1e-5, defect)
        out[c] = z[c].astype(np.float64) * np.float64(sc) + np.float64(sh)
    return out


def _error(pr, y, got):
    ref = P.sums_of(y, pr.table)
    g = P.sums_of(got, pr.table)
    return float("inf") if not np.isfinite(g).all() else float(np.abs(g - ref).max() / max(1.0, np.abs(ref).max()))


def _channels(pr, *regimes):
    return [c for c, r in enumerate(pr.regimes) if r in regimes]


def test_the_model_itself_meets_the_bound(model_parts):
    pr, z, y, base = model_parts
    err = _error(pr, y, base)
    print("tiled fp32 statistics model, no defect: %.2e of %.0e" % (err, pr.tol))
    assert err <= 0.25 * pr.tol


@pytest.mark.parametrize("defect,regimes", [("a", ("offset+", "offset-")), ("b", ("offset+", "offset-")), ("d", ("small",)), ("e", ("big",))])
def test_planted_defect_is_rejected_by_its_regime(model_parts, defect, regimes):
    """the defect in the channels of the named regime ONLY, every other channel as the float64 reference has it"""
    pr, z, y, _ = model_parts
    err = _error(pr, y, _model_output(pr, z, defect, _channels(pr, *regimes), y))
    print("defect (%s) in the %s channels: %.1f x the tolerance" % (defect, " / ".join(regimes), err / pr.tol))
    assert err > pr.tol
    with pytest.raises(AssertionError):
        P.assert_close(P.sums_of(_model_output(pr, z, defect, _channels(pr, *regimes), y), pr.table), P.sums_of(y, pr.table), pr.tol, "mutant")


@pytest.mark.parametrize("defect", ["a", "b", "e"])
def test_planted_defect_is_accepted_on_plain_channels_alone(model_parts, defect):
    """... which is all the suite had: the same defects in the plain channels stay inside the bound"""
    pr, z, y, _ = model_parts
    err = _error(pr, y, _model_output(pr, z, defect, _channels(pr, "plain"), y))
    print("defect (%s) in the plain channels: %.2f x the tolerance" % (defect, err / pr.tol))
    assert err <= pr.tol


def test_defect_c_a_missing_clamp_cannot_be_seen_at_these_magnitudes(model_parts):
    """NOT what was hoped for (module docstring): without the clamp the model gives the very same scale and shift in every channel of
    every regime, the flat ones included -- their variance is exactly zero, not negative"""
    pr, z, _, _ = model_parts
    flat = _channels(pr, "flat")
    assert flat and all(np.ptp(z[c]) == 0 for c in flat)
    for c in range(z.shape[0]):
        assert tiled_scale_shift(z[c], 1.0, pr.B, 1e-5, "c") == tiled_scale_shift(z[c], 1.0, pr.B, 1e-5, None), (c, pr.regimes[c])
    # the flat regime does check what a constant channel can check: the reference output is exactly beta, and the model's is within
    # (fp32 rounding of the mean and of the shift) / sqrt(eps)
    sc, sh = tiled_scale_shift(z[flat[0]], 1.0, pr.B, 1e-5)
    assert abs(float(z[flat[0]][0, 0]) * float(sc) + float(sh) - pr.B) <= 2.0 ** -24 * (abs(pr.B) + 0.5 / np.sqrt(1e-5)) * 2
