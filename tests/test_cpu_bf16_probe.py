"""The bf16-exact probes of tests/util/layer_probe.py ("bf16-exact probes"), without a GPU: every case of tests/test_gpu_bf16_parity.py
builds, everything its convolutions under test read is a bf16 number in the float64 reference, the stream-K cases have the unit counts
that cut tiles, the reference agrees with the fp32 oracle's bf16-operand mode, and the comparison rejects five defects a bf16-operand
kernel, its launch or the host's weight copy can have -- each planted into the REFERENCE, the factor by which it exceeds the case's
tolerance printed."""
import copy
import os
import sys

import numpy as np
import pytest
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import layer_probe as P  # noqa: E402
from fav_amd import t7  # noqa: E402

ALL = P.BF16_CASES + P.BF16_SK_CASES
VARIANTS = ("stats", "raw")


def _case(name):
    return next(c for c in ALL if c["name"] == name)


def _own(pr):
    """L's convolutions in the reference's layer list"""
    return P.conv_layers(pr.ref_layers)[pr.conv0:pr.conv0 + len(pr.ids)]


def test_case_names_are_unique_and_both_filter_counts_and_stage_counts_are_asked_for():
    names = [c["name"] for c in ALL]
    assert len(set(names)) == len(names)
    assert {i for c in ALL for i in c["ids"]} == {364, 428}
    for n in (64, 128): assert any("U2,c3s1-%d" % n in c["arch"] for c in ALL)      # <n, true>: two pending stages


@pytest.mark.parametrize("case", ALL, ids=lambda c: c["name"])
def test_probe_builds_and_what_the_kernel_reads_is_bf16(tmp_path, case):
    for variant in VARIANTS:
        pr = P.probe_for(case, variant, tmp_path)
        n = len(pr.ids)
        ins = P.bf16_conv_inputs(pr.ref_layers, pr.x)[pr.conv0:pr.conv0 + n]
        for a in ins:
            assert P.is_bf16(a)
            assert (a != 0).mean() > 0.3 and len(np.unique(a)) > 16               # ... and not trivially so
        own = _own(pr)
        for L in own: assert P.is_bf16(L["w"])                                      # the reference convolves with bf16 weights,
        last = P.conv_layers(pr.layers)[pr.conv0 + n - 1]["w"]
        assert np.mean(P.conv_layers(pr.ref_layers)[pr.conv0 + n - 1]["w"] != last) > 0.9      # which the checkpoint's are not
        # the norms in front of L: the library's fp32 scale (net_model.cpp: gamma / sqrt(var + eps) in double, then float) is the intended number
        for Lr, Lo in zip(P.front_norms(pr.ref_layers, pr.conv0, n), P.front_norms(pr.layers, pr.conv0, n)):
            sc = (Lo["gamma"].astype(np.float64) / np.sqrt(Lo["var"].astype(np.float64) + np.float64(np.float32(Lo["eps"])))).astype(np.float32)
            assert np.all(np.abs(sc.astype(np.float64) - Lr["gamma"]) <= np.spacing(np.abs(Lr["gamma"]).astype(np.float32)))
            assert np.array_equal(Lo["beta"], np.round(Lo["beta"])) and not np.any(Lo["mean"])
            assert len(set(Lr["gamma"].tolist())) >= 5
            C = len(Lr["gamma"])
            if C >= 64: assert np.all((Lr["gamma"][:32] != Lr["gamma"][32:64]) | (Lr["beta"][:32] != Lr["beta"][32:64]))
        for p, path in enumerate(pr.paths):
            layers = P.bf16_reference_layers(t7.extract_layers(t7.load(path)["model"]), pr.conv0, n)
            _, pre, arg = P.reference_parts(layers, pr.x)
            if pre is not None: assert pre.min() >= 1.0, (variant, pre.min())        # the ReLU in front of the observer is the identity
            assert 0.05 <= np.abs(arg).max() <= 0.5, (variant, np.abs(arg).max())
            obs = layers[max(i for i, L in enumerate(layers) if L["type"] == "conv")]
            assert np.array_equal(obs["w"], P.observer_weights(pr.table, p)) and not np.any(obs["b"])
        assert tuple(arg.shape[1:]) == tuple(case["out"])
        assert pr.tol == (P.TOL_STATS if variant == "stats" else P.TOL_RAW)


def test_stream_k_cases_cut_their_tiles():
    """launch_h3_t: grid = 1 below nres units, else nres blocks with units U * b / nres ... -- from 257 units on (256 CUs) and off the
    multiples of 256 every tile's units (cin / 32 x 3 tap rows) are spread over several blocks and ranges start mid-slice.  The other
    cases stay below: one block does everything, which is their point"""
    for c in P.BF16_SK_CASES:
        u = P.bf16_units(c)
        assert u >= 257 and u % 256 != 0, (c["name"], u)
        per_tile = u // (-(-c["out"][0] // 8) * -(-c["out"][1] // 32))
        starts = {(u * b // 256) % per_tile % 3 for b in range(256)}
        assert starts == {0, 1, 2}, starts                                          # ky0 = 1 and 2: the prologue's q1 pieces
        assert len({(u * b // 256) // per_tile for b in range(256)}) == u // per_tile      # every tile is shared
    assert P.bf16_units(_case("bf16_sk_256_128")) == 12 * 24 and P.bf16_units(_case("bf16_sk_R128")) == 24 * 12
    for c in P.BF16_CASES: assert P.bf16_units(c) < 104                            # (a quarter of a small device would still take grid = 1)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c["name"])
def test_reference_agrees_with_the_fp32_oracle_in_bf16_operand_mode(oracle, tmp_path, case):
    """oracle.net_forward(bf16_ops=True) on the very checkpoints the GPU loads: it rounds both operands of exactly L's convolutions, and
    through the observer it meets the float64 reference far inside TOL_RAW"""
    for variant in VARIANTS:
        pr = P.probe_for(case, variant, tmp_path)
        marked = [i for i, L in enumerate(P.conv_layers(pr.layers)) if oracle._bf16_conv(L)]
        assert marked == list(range(pr.conv0, pr.conv0 + len(pr.ids))), marked
        outs = [oracle.net_forward(t7.extract_layers(t7.load(path)["model"]), pr.x, bf16_ops=True) for path in pr.paths]
        ref = P.reference_sums(pr.ref_layers, pr.x, pr.table)
        err = P.assert_close(P.observe(outs, pr.table), ref, P.TOL_RAW, case["name"])
        print("bf16 probe %-22s %-5s fp32 oracle (bf16 operands) vs float64: %.2e of %.0e" % (case["name"], variant, err, P.TOL_RAW))
        assert err <= 0.1 * P.TOL_RAW


# ------------------------------------------------------------------------------------------------ mutation control
def _factor(pr, mutant_y):
    """by how many tolerances the observed sums of a mutant move; the comparison must reject it"""
    ref = P.reference_sums(pr.ref_layers, pr.x, pr.table)
    got = P.sums_of(mutant_y, pr.table)
    with pytest.raises(AssertionError):
        P.assert_close(got, ref, pr.tol, "mutant")
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) / pr.tol


def _observed(pr, layers):
    return P.reference_parts(layers, pr.x)[0]


def _with_weights(pr, f):
    ls = copy.deepcopy(pr.ref_layers)
    for Lm, Lo in zip(P.conv_layers(ls)[pr.conv0:pr.conv0 + len(pr.ids)], P.conv_layers(pr.layers)[pr.conv0:pr.conv0 + len(pr.ids)]):
        Lm["w"] = f(Lo["w"])
    return ls


@pytest.mark.parametrize("case", ALL, ids=lambda c: c["name"])
def test_mutant_weights_not_rounded_to_nearest_even(tmp_path, case):
    """(a) the fp32 weights as they are -- the fp32 kernel ran, or the copy was never rounded; (b) truncated to bf16 instead of rounded"""
    for variant in VARIANTS:
        pr = P.probe_for(case, variant, tmp_path)
        fa = _factor(pr, _observed(pr, _with_weights(pr, lambda w: w)))
        fb = _factor(pr, _observed(pr, _with_weights(pr, lambda w: (w.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32))))
        print("bf16 mutant %-22s %-5s fp32 weights %.1f x, truncated weights %.1f x the tolerance" % (case["name"], variant, fa, fb))
        assert fa >= 2 and fb >= 2


def _split(pr):
    """a case whose L is one top-level convolution: (index of L in the layer list, its float64 input, its raw output z)"""
    ls = pr.ref_layers
    own = _own(pr)[0]
    i = next(i for i, L in enumerate(ls) if L is own)
    tr = []
    P.forward64(ls, P._t64(pr.x), tr)
    return i, tr[i - 1][1], tr[i][1].numpy()


def _behind(pr, i, z):
    """L's raw output -> the observed tensor"""
    tr = []
    P.forward64(pr.ref_layers[i + 1:], P._t64(z), tr)
    return tr[P.observed_index([t for t, _ in tr])][1].numpy()


@pytest.mark.parametrize("variant", VARIANTS)
def test_mutant_halo_column_between_two_tiles_zeroed(tmp_path, variant):
    """(c) one column of ONE tile's halo staged as zeros.  L is zero-padded by 1: the tile of output columns 32..63 reads input columns
    31..64 and the tile 0..31 reads -1..32, so input column 32 is the last halo column of the first tile (only output column 31 meets it
    there) and 31 the first of the second (output column 32)"""
    pr = P.probe_for(_case("bf16_64_ragged"), variant, tmp_path)
    i, xin, z = _split(pr)
    conv = pr.ref_layers[i]
    assert conv["pad"] == 1 and np.abs(_behind(pr, i, z) - _observed(pr, pr.ref_layers)).max() < 1e-9
    for col, out_col, rows in ((32, 31, slice(0, 8)), (31, 32, slice(8, 16))):
        xm = xin.clone(); xm[:, :, col] = 0
        zm = F.conv2d(xm[None], P._t64(conv["w"]), P._t64(conv["b"]), stride=1, padding=1)[0].numpy()
        m = z.copy(); m[:, rows, out_col] = zm[:, rows, out_col]                       # one tile: 8 rows of one output column
        f = _factor(pr, _behind(pr, i, m))
        print("bf16 mutant input column %d zeroed in one tile's halo (%s): %.1f x the tolerance" % (col, variant, f))
        assert f >= 2


@pytest.mark.parametrize("name", ["bf16_R128_ragged", "bf16_128_U2", "bf16_sk_256_128"])
def test_mutant_second_channel_slice_takes_the_first_one_s_scale_and_shift(tmp_path, name):
    """(d) aff[] of channels 32..63 read from 0..31 (the norm directly in front of L's last convolution; with two pending stages: either)"""
    for variant in VARIANTS:
        pr = P.probe_for(_case(name), variant, tmp_path)
        for which in range(len(P.front_norms(pr.ref_layers, pr.conv0, len(pr.ids)))):
            ls = copy.deepcopy(pr.ref_layers)
            bn = P.front_norms(ls, pr.conv0, len(pr.ids))[which]
            if len(bn["gamma"]) < 64: continue
            if name == "bf16_R128_ragged" and which == 0: continue                    # (the prefix norm feeds the skip as well: not this defect)
            for k in ("gamma", "beta"): bn[k][32:64] = bn[k][0:32]
            f = _factor(pr, _observed(pr, ls))
            print("bf16 mutant %-18s %-5s norm %d: channels 32..63 with the scale / shift of 0..31: %.1f x the tolerance" % (name, variant, which, f))
            assert f >= 2


def test_mutant_one_tile_s_pixel_count_wrong(tmp_path):
    """(e) the epilogue of the 8 x 20 tile at the right edge takes cnt = 256: its mean and M2 are formed with it and in_finalize adds
    n mu and M2 + n mu^2 with it (kernels_elem.hip) -- the sum stays right, the sum of squares gets sum^2 (n - cnt) / cnt^2"""
    pr = P.probe_for(_case("bf16_64_no_edge_tiles"), "stats", tmp_path)
    i, _, z = _split(pr)
    assert pr.ref_layers[i + 1]["type"] == "in" and z.shape[1:] == (9, 52)
    C, M = z.shape[0], z.shape[1] * z.shape[2]
    tile = z[:, 0:8, 32:52].reshape(C, -1)
    n, cnt = tile.shape[1], 256
    s1 = z.reshape(C, -1).sum(axis=1)
    s2 = (z.reshape(C, -1) ** 2).sum(axis=1) + tile.sum(axis=1) ** 2 * (n - cnt) / cnt ** 2
    mean, var = s1 / M, np.maximum(s2 / M - (s1 / M) ** 2, 0)
    m = (z - mean[:, None, None]) / np.sqrt(var + pr.ref_layers[i + 1]["eps"])[:, None, None] + pr.B
    y = _observed(pr, pr.ref_layers)
    right = (z - z.mean(axis=(1, 2), keepdims=True)) / np.sqrt(z.var(axis=(1, 2), keepdims=True) + pr.ref_layers[i + 1]["eps"]) + pr.B
    assert np.abs(right - y).max() < 1e-9                                            # (the helper restates the norm)
    f = _factor(pr, m)
    print("bf16 mutant one tile counted as full in the statistics: %.1f x the tolerance" % f)
    assert f >= 2
