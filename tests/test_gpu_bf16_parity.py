"""Per-kernel parity of the bf16-operand fast mode (-m gpu): conv3_halo_bf16_kernel<BN, S2> (fav_net_set_precision), observed through the
identity tail of tests/util/layer_probe.py on bf16-exact probes.  Everything the kernel reads is a bf16 number in the float64 reference
and its weights are the reference's bf16_round(w), so its operand rounding is the identity, every product is exact in fp32, and it has to
meet the float64 convolution at the project's ordinary per-kernel tolerances: 2e-4 x max(1, max |ref|) for a convolution ("raw"), 5e-4 x
for convolution + InstanceNorm ("stats": the kernel's partials / counts epilogue), on every observed group sum.  The cases: every
instantiation, sub-tile / one-tile / ragged sizes, padding layers in front, padded filter counts, stream-K with cut tiles (also
NaN-poisoned, and once more as one block per tile), and the fp32 mode's bits on either side of a switch.  Every case prints its
normalised error (profiles/bf16_parity.log); tests/test_cpu_bf16_probe.py has the probes' own checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import layer_probe as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _forward(favlib, cuda, pr, shared=False):
    """test_gpu_layer_parity.py's _forward in the fast mode: every pass of a probe through a fresh network with bf16 operands (optionally
    one block per tile: fav_net_set_shared_device); the kernel ids of L's convolutions from the first.  net.check() after each forward:
    a stream-K hand-off that times out reports through it instead of hanging"""
    import torch
    x = torch.from_numpy(pr.x).to(cuda)
    outs = []
    for p, path in enumerate(pr.paths):
        net = favlib.Net(path, 0)
        net.set_precision(True)
        if shared: net.set_shared_device(True)
        if p == 0: net.profile_enable(True)
        outs.append(net.forward(x).cpu().numpy())
        net.check()
        if p == 0:
            prof = net.profile_read()
            assert [prof[pr.conv0 + i][3] for i in range(len(pr.ids))] == pr.ids, ([r[3] for r in prof], pr.conv0, pr.ids)
        net.close()
    return outs


def _compare(case, variant, pr, outs, tag=""):
    ref = P.reference_sums(pr.ref_layers, pr.x, pr.table)
    err = P.assert_close(P.observe(outs, pr.table), ref, pr.tol, "%s %s%s" % (case["name"], variant, tag))
    print("bf16_parity %-22s %-5s%s kernel %-7s out %3dx%-3d units %3d max|ref| %8.3f  err %.2e of %.0e"
          % (case["name"], variant, tag, "/".join(str(i) for i in pr.ids), case["out"][0], case["out"][1], P.bf16_units(case), np.abs(ref).max(), err, pr.tol))


@pytest.mark.parametrize("case", P.BF16_CASES + P.BF16_SK_CASES, ids=lambda c: c["name"])
def test_bf16_kernel_matches_float64(favlib, cuda, poison, tmp_path, case):
    for variant in ("stats", "raw"):
        pr = P.probe_for(case, variant, tmp_path)
        _compare(case, variant, pr, _forward(favlib, cuda, pr))
        if case["poison"]:      # nothing the kernel reads -- LDS, the hand-off workspace and its flags -- may be left over from before
            poison()
            _compare(case, variant, pr, _forward(favlib, cuda, pr), " (poisoned)")


@pytest.mark.parametrize("case", P.BF16_SK_CASES[:1], ids=lambda c: c["name"])
def test_bf16_kernel_one_block_per_tile_matches_float64(favlib, cuda, tmp_path, case):
    """the same ragged stream-K case as data-parallel tiles (no_sk): the same reference, the same tolerance"""
    for variant in ("stats", "raw"):
        pr = P.probe_for(case, variant, tmp_path)
        _compare(case, variant, pr, _forward(favlib, cuda, pr, shared=True), " (one block per tile)")


def test_fp32_bits_survive_a_switch_to_bf16_and_back(favlib, cuda, tmp_path):
    """fp32, bf16, fp32 on one network at the largest stream-K case (the two modes tile and size their statistics buffers differently: the
    arena is rebuilt at each switch): the fp32 outputs are bit-equal, and the bf16 one in between meets the reference"""
    import torch
    case = next(c for c in P.BF16_SK_CASES if c["name"] == "bf16_sk_R128")
    pr = P.probe_for(case, "stats", tmp_path)
    x = torch.from_numpy(pr.x).to(cuda)
    nets = [favlib.Net(path, 0) for path in pr.paths]
    a = [net.forward(x).cpu().numpy() for net in nets]
    for net in nets: net.check(); net.set_precision(True)
    mid = [net.forward(x).cpu().numpy() for net in nets]
    for net in nets: net.check(); net.set_precision(False)
    b = [net.forward(x).cpu().numpy() for net in nets]
    for net in nets: net.check(); net.close()
    for p in range(len(nets)):
        assert np.array_equal(a[p].view(np.uint32), b[p].view(np.uint32)), "pass %d: fp32 output changed across a precision switch" % p
    _compare(case, "stats", pr, mid, " (between two fp32 forwards)")
    assert any(not np.array_equal(a[p], mid[p]) for p in range(len(nets)))      # (the switch did select other arithmetic)
