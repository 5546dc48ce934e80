"""InstanceNorm statistics at the numeric edges (-m gpu): every kernel that writes statistics -- the convolution epilogues, the F(4x4)
kernel's accumulator form and its partials form, stats_kernel and res_add_stats_kernel -- and the three consumers that turn them into
scale and shift, with the output channels of the layer under test by turns plain, offset by +-2^9 sigma, of RMS 2^10..2^11, of
sigma 2^-9..2^-8 and constant (tests/util/layer_probe.py, REGIMES; tests/test_cpu_stats_edges.py shows what each is there for).

The identity-tail probe of tests/test_gpu_layer_parity.py, "stats" variant, at each family's ragged size and its one-tile size where a
full tile matters; the float64 model of the very checkpoint is the reference and the bound is the project's own, unchanged:
TOL_STATS = 5e-4 x max(1, max |ref|) on the observed group sums.  Every case asserts its kernel ids and prints its normalised error
(profiles/stats_edges.log)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import layer_probe as P  # noqa: E402
import test_gpu_layer_parity as LP  # noqa: E402  (the forward / child-process helpers: one scheme for both files)

pytestmark = pytest.mark.gpu


def _compare(case, pr, outs, tag=""):
    ref = P.reference_sums(pr.layers, pr.x, pr.table)
    assert pr.tol == P.TOL_STATS
    got = P.observe(outs, pr.table)
    # printed before it is asserted: a failing case leaves its figure in the log
    err = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if np.isfinite(got).all() else float("nan")
    print("stats_edges %-24s%s kernel %-9s out %3dx%-3d max|ref| %8.3f  err %.2e of %.0e"
          % (case["name"], tag, "/".join(str(i) for i in pr.ids) or "-", case["out"][0], case["out"][1], np.abs(ref).max(), err, pr.tol))
    P.assert_close(got, ref, pr.tol, "%s%s" % (case["name"], tag))


@pytest.mark.parametrize("case", P.EDGE_CASES + P.ELEMENT_CASES, ids=lambda c: c["name"])
def test_statistics_match_float64_under_the_regimes(favlib, cuda, poison, tmp_path, case):
    pr = P.probe_for(case, "stats", tmp_path, regimes=True)
    _compare(case, pr, LP._forward(favlib, cuda, pr))
    if case["poison"]:
        poison()
        _compare(case, pr, LP._forward(favlib, cuda, pr), " (poisoned)")


def _children(tmp_path, env, cases, label):
    probes = []
    for case in cases:
        pr = P.probe_for(case, "stats", tmp_path, regimes=True)
        stem = str(tmp_path / case["name"])
        np.save(stem + "_x.npy", pr.x)
        probes.append((case, "stats", pr, stem))
    LP._run_child(tmp_path, env, probes, "")
    import json
    for case, _, pr, stem in probes:
        ids = json.load(open(stem + "_ids.json"))
        assert ids[pr.conv0:pr.conv0 + len(pr.ids)] == pr.ids, (case["name"], ids, pr.conv0)
        _compare(case, pr, [np.load(stem + "_out%d.npy" % p) for p in range(len(pr.paths))], label)


@pytest.mark.parametrize("group", P.EDGE_DIAG_CASES, ids=lambda g: "+".join(sorted(k[4:] for k in g[0])))
def test_statistics_match_float64_behind_the_diagnostic_switches(favlib, cuda, tmp_path, group):
    """FIRST1D, S2HALO, GENERIC 128 / 64 / 32, C8D, C8, WINO F(2x2), the stream-K shares and the pending join: one child per switch set"""
    env, cases = group
    _children(tmp_path, env, cases, " (diag)")


def test_f4x4_statistics_in_the_partials_form(favlib, cuda, tmp_path):
    """the F(4x4) cases of the first test once more with every InstanceNorm through partials + in_finalize_kernel: both forms meet the
    bound, so a defect of the accumulator form and one of the unit statistics would show apart"""
    _children(tmp_path, P.EDGE_PARTIALS_ENV, P.EDGE_PARTIALS_CASES, " (partials)")
