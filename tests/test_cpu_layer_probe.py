"""The layer probe of tests/util/layer_probe.py, without a GPU: the observer recovers a layer's output from the network's output (shown
with the fp32 C oracle standing in for the GPU), every case of the GPU table meets the probe's two conditions in the float64 reference,
and the comparison rejects four small, local defects of the kind a convolution kernel or its statistics epilogue can have."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import layer_probe as P  # noqa: E402
from fav_amd import t7  # noqa: E402

ALL_CASES = P.CASES + [c for _, cs in P.DIAG_CASES for c in cs]


def _case(name):
    return next(c for c in ALL_CASES if c["name"] == name)


def test_case_names_are_unique_and_every_kernel_id_is_asked_for():
    names = [c["name"] for c in ALL_CASES]
    assert len(set(names)) == len(names)
    ids = {i for c in ALL_CASES for i in c["ids"]}
    # fav_internal.h, enum ConvKernel: FOLD, FIRST1D, C8D, C8, FIRST2D, GENERIC x 3, S2HALO, HALO3, WINO, UP2, WINO4 (+ pending join), S2W, TCONV
    assert {1, 6, 7, 8, 16, 32, 64, 128, 264, 364, 428, 528, 564, 628, 756, 728, 729, 856, 764, 828, 956, 832} <= ids


@pytest.mark.parametrize("name", ["first2d_7_32_small", "halo3_32_64_small", "pad_replicate", "wino4_R128_small", "tconv_64_32", "fold_32_small", "fold_32_U2"])
@pytest.mark.parametrize("variant", ["stats", "raw"])
def test_probe_is_sound(oracle, tmp_path, name, variant):
    """the fp32 oracle pushed through the observer: the recovered sums are the oracle's own tensor in front of the observer, summed by
    the table, to a few fp32 ulp of the summands -- and they meet the float64 reference far inside the GPU tolerance"""
    pr = P.probe_for(_case(name), variant, tmp_path)
    outs, want = [], None
    for path in pr.paths:
        layers = t7.extract_layers(t7.load(path)["model"])
        tr = []
        outs.append(oracle.net_forward(layers, pr.x, tr))
        if want is None:
            types = [t for t, _ in tr]
            want = tr[max(i for i, t in enumerate(types) if t == "conv")][1] if pr.direct else P.sums_of(tr[P.observed_index(types)][1], pr.table)
    got = P.observe(outs, pr.table)
    # Element by element, relative to the value itself.  The oracle's observer accumulates in double (exact for <= 8 fp32 summands times
    # 2^-k) and rounds once: 1/2 ulp = 2^-24.  tanhf: <= 2 ulp = 4 x 2^-24.  The product with 150: 2^-24.  Six units of 2^-24 relative in the
    # network's output; atanh in float64 turns a relative error of t into (t / atanh t) / (1 - t^2) <= 1.18 times as much of the
    # argument for |argument| <= 0.5: 7.1 x 2^-24, asked as 8 (four fp32 ulp)
    assert np.all(np.abs(got - want) <= 8 * 2.0 ** -24 * np.abs(want)), float((np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max() * 2.0 ** 24)
    ref = P.reference_sums(pr.layers, pr.x, pr.table)
    err = P.assert_close(got, ref, pr.tol, name)
    print("probe soundness %-22s %-5s B %4.1f k %d  fp32 oracle vs float64: %.2e of %.0e" % (name, variant, pr.B, pr.table["k"], err, pr.tol))
    assert err <= 0.1 * pr.tol


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_conditions_hold_for_every_gpu_case(tmp_path, case):
    """conditions, not tolerances: in the float64 reference the ReLU behind L is the identity (every pre-ReLU value >= 1), the tanh
    argument stays within 0.5, and the observer's weights are the table's (every channel of L in exactly one group)"""
    for variant in ("stats", "raw"):
        pr = P.probe_for(case, variant, tmp_path)
        seen = np.zeros(pr.table["channels"], int)
        for p, path in enumerate(pr.paths):
            layers = t7.extract_layers(t7.load(path)["model"])
            _, pre, arg = P.reference_parts(layers, pr.x)
            if pre is not None and not pr.direct: assert pre.min() >= 1.0, (variant, pre.min())      # (direct: the ReLU in front of L is an ordinary one)
            assert np.abs(arg).max() <= 0.5, (variant, np.abs(arg).max())
            assert np.abs(arg).max() >= 0.05                  # ... and the observed signal is not thrown away either
            if pr.direct: continue
            obs = layers[max(i for i, L in enumerate(layers) if L["type"] == "conv")]
            assert np.array_equal(obs["w"], P.observer_weights(pr.table, p)) and not np.any(obs["b"])
            for g, _ in pr.table["passes"][p]: seen[g] += 1
        assert pr.direct or np.all(seen == 1)
        assert tuple(arg.shape[1:]) == tuple(case["out"])     # L's output has the size the case names (the observer keeps it)


# ------------------------------------------------------------------------------------------------ mutation control
def _parts(tmp_path, name, variant):
    """the float64 pieces of a case whose L is a 3x3 convolution: its input, weights, bias, raw output z, and the observed tensor y"""
    pr = P.probe_for(_case(name), variant, tmp_path)
    tr = []
    P.forward64(pr.layers, P._t64(pr.x), tr)
    types = [t for t, _ in tr]
    j = P.observed_index(types)                           # the ReLU behind L's norm
    assert types[j] == "relu" and types[j - 2] == "conv"
    conv = pr.layers[j - 2]
    return pr, tr[j - 3][1], conv, tr[j - 2][1].numpy(), tr[j][1].numpy()


def _renorm(pr, z):
    """L's raw output -> the observed tensor, as the norm behind L maps it"""
    if pr.variant == "raw": return z / np.sqrt(np.float64(np.float32(1.0 - 1e-5)) + 1e-5) + pr.B
    return P.instnorm64(torch.from_numpy(z), torch.ones(z.shape[0], dtype=torch.float64), torch.full((z.shape[0],), pr.B, dtype=torch.float64), 1e-5).numpy()


def _rejected(pr, ref_y, mutant_y):
    ref = P.sums_of(ref_y, pr.table)
    with pytest.raises(AssertionError):
        P.assert_close(P.sums_of(mutant_y, pr.table), ref, pr.tol, "mutant")
    P.assert_close(ref, ref, pr.tol)
    return float(np.abs(P.sums_of(mutant_y, pr.table) - ref).max() / max(1.0, np.abs(ref).max())) / pr.tol


@pytest.mark.parametrize("variant", ["stats", "raw"])
def test_mutant_one_pixel_moved(tmp_path, variant):
    pr, _, _, z, y = _parts(tmp_path, "halo3_32_64_ragged", variant)
    assert np.abs(_renorm(pr, z) - y).max() < 1e-9          # (the helper restates the norm)
    m = y.copy()
    c = 37
    m[c, 5, 7] += 1e-2 * y[c].std()
    print("one pixel moved by 1e-2 sigma: %.1f x the tolerance" % _rejected(pr, y, m))


@pytest.mark.parametrize("variant", ["stats", "raw"])
def test_mutant_one_tap_dropped_in_the_last_column(tmp_path, variant):
    pr, xin, conv, z, y = _parts(tmp_path, "halo3_32_64_ragged", variant)
    # (the layer is zero-padded: in the last column the tap right of the centre reads zeros anyway, so the one left of it goes)
    w = P._t64(conv["w"]).clone(); w[:, :, 1, 0] = 0
    zm = F.conv2d(xin[None], w, P._t64(conv["b"]), stride=1, padding=conv["pad"])[0].numpy()
    m = z.copy(); m[:, :, -1] = zm[:, :, -1]
    print("one tap dropped in the last column: %.1f x the tolerance" % _rejected(pr, y, _renorm(pr, m)))


def test_mutant_ragged_tile_row_left_out_of_the_variance(tmp_path):
    pr, _, _, z, y = _parts(tmp_path, "halo3_32_64_ragged", "stats")
    assert z.shape[1] % 8 == 1                               # 8-row tiles: the last row is the ragged one
    c = 11
    mean = z[c].mean()
    var = ((z[c, :-1] - mean) ** 2).mean()                   # that tile's rows never reached the sum of squares
    m = y.copy()
    m[c] = (z[c] - mean) / np.sqrt(var + 1e-5) + pr.B
    print("ragged tile row left out of one channel's variance: %.1f x the tolerance" % _rejected(pr, y, m))


def test_mutant_bias_dropped(tmp_path):
    pr, _, conv, z, y = _parts(tmp_path, "halo3_32_64_ragged", "raw")
    c = int(np.argmax(np.abs(conv["b"])))
    m = z.copy(); m[c] -= np.float64(conv["b"][c])
    print("one channel's bias (%.3f) dropped: %.1f x the tolerance" % (conv["b"][c], _rejected(pr, y, _renorm(pr, m))))
