"""Per-kernel parity (-m gpu): every convolution kernel of libfav, and the statistics its epilogue writes, observed through an identity
tail (tests/util/layer_probe.py) and compared with a float64 model of the same checkpoint.

Each case names the kernel its layer must run on (profile ids: csrc/fav_internal.h, enum ConvKernel) and runs two variants: "stats" --
the layer's InstanceNorm with gamma 1, beta B in front of a ReLU that B makes the identity -- and "raw" -- an evaluate-mode BatchNorm
that only shifts, so the bias is seen.  Tolerances are the project's own (test_gpu_parity.py): 2e-4 x max(1, max |ref|) for a
convolution, 5e-4 x for convolution + InstanceNorm, on the observed group sums; nothing per kernel.  Every case prints its normalised
error (profiles/layer_parity.log)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import layer_probe as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "fast-artistic-videos_amd", "libfav_diag.so")

pytestmark = pytest.mark.gpu


def _forward(favlib, cuda, pr):
    """every pass of a probe through a fresh network; the kernel ids of L's convolutions from the first"""
    import torch
    x = torch.from_numpy(pr.x).to(cuda)
    outs = []
    for p, path in enumerate(pr.paths):
        net = favlib.Net(path, 0)
        if p == 0: net.profile_enable(True)
        outs.append(net.forward(x).cpu().numpy())
        net.check()
        if p == 0:
            prof = net.profile_read()
            assert [prof[pr.conv0 + i][3] for i in range(len(pr.ids))] == pr.ids, ([r[3] for r in prof], pr.conv0, pr.ids)
        net.close()
    return outs


def _compare(case, variant, pr, outs, tag=""):
    ref = P.reference_sums(pr.layers, pr.x, pr.table)
    err = P.assert_close(P.observe(outs, pr.table), ref, pr.tol, "%s %s%s" % (case["name"], variant, tag))
    print("layer_parity %-24s %-5s%s kernel %-9s out %3dx%-3d max|ref| %8.3f  err %.2e of %.0e"
          % (case["name"], variant, tag, "/".join(str(i) for i in pr.ids), case["out"][0], case["out"][1], np.abs(ref).max(), err, pr.tol))


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c["name"])
def test_layer_matches_float64(favlib, cuda, poison, tmp_path, case):
    for variant in ("stats", "raw"):
        pr = P.probe_for(case, variant, tmp_path)
        _compare(case, variant, pr, _forward(favlib, cuda, pr))
        if case["poison"]:      # nothing the kernel reads may be left over from whoever had the GPU before
            poison()
            _compare(case, variant, pr, _forward(favlib, cuda, pr), " (poisoned)")


CHILD = """
import json, sys, numpy as np, torch
sys.path.insert(0, %r)
import fav_amd
for job in json.load(open(sys.argv[1])):
    x = torch.from_numpy(np.load(job["x"])).cuda()
    for p, path in enumerate(job["paths"]):
        net = fav_amd.Net(path, 0)
        if p == 0: net.profile_enable(True)
        np.save(job["out"] %% p, net.forward(x).cpu().numpy())
        net.check()
        if p == 0: json.dump([r[3] for r in net.profile_read()], open(job["ids"], "w"))
        net.close()
""" % os.path.join(ROOT, "fast-artistic-videos_amd", "python")


def _run_child(tmp_path, env, probes, tag):
    """one child process on the diagnostic library: every pass of every probe; returns nothing, the outputs are files next to the stems"""
    jobs = [{"x": stem + "_x.npy", "paths": pr.paths, "out": stem + tag + "_out%d.npy", "ids": stem + tag + "_ids.json"} for _, _, pr, stem in probes]
    json.dump(jobs, open(tmp_path / ("jobs%s.json" % tag), "w"))
    subprocess.check_call([sys.executable, "-c", CHILD, str(tmp_path / ("jobs%s.json" % tag))], env=dict(os.environ, FAV_AMD_LIB=DIAG_LIB, **env), timeout=300)


def _check_child(probes, tag, label=""):
    for case, variant, pr, stem in probes:
        ids = json.load(open(stem + tag + "_ids.json"))
        assert ids[pr.conv0:pr.conv0 + len(pr.ids)] == pr.ids, (case["name"], variant, ids, pr.conv0)
        _compare(case, variant, pr, [np.load(stem + tag + "_out%d.npy" % p) for p in range(len(pr.paths))], label)


@pytest.mark.parametrize("group", P.DIAG_CASES, ids=lambda g: "+".join(sorted(k[4:] for k in g[0])))
def test_layer_matches_float64_behind_the_diagnostic_switches(favlib, cuda, poison, tmp_path, group):
    """the kernels only the diagnostic library selects (the switches are read once per process: one child per set of them), at the same
    three sizes per kernel; the cases marked for it once more in a second child that starts behind NaN-poisoned LDS and memory"""
    env, cases = group
    probes = []
    for case in cases:
        for variant in ("stats", "raw"):
            pr = P.probe_for(case, variant, tmp_path)
            stem = str(tmp_path / ("%s_%s" % (case["name"], variant)))
            np.save(stem + "_x.npy", pr.x)
            probes.append((case, variant, pr, stem))
    _run_child(tmp_path, env, probes, "")
    _check_child(probes, "")
    again = [q for q in probes if q[0]["poison"]]
    assert again
    poison()
    _run_child(tmp_path, env, again, "_poisoned")
    _check_child(again, "_poisoned", " (poisoned)")
