"""A/B of the estimator's four variants on one 1280x720 pair, on one GPU:
  bright       default options (brightness constancy, quadratic smoothness)
  eps0.3       smooth_eps 0.3: the edge weights, the weighted sweeps
  grad         data_term 1: the five-plane coefficients with their 13-point warp stencil, the tensor sweeps
  grad+eps0.3  both
every one through fav_flow_rgb8_ex, and on this build only, through fav_flow_rgb8_ex2,
  match              match_beta -1 (the default weight): the matching prior on the default estimator
  match+grad+eps0.3  the prior with both other options
with the prior's own launches timed on their own at the level-1 size (fav_flow_match_f32: both directions in one launch; then
fav_flow_match_check).  synth.smooth_frame inputs (the second image is the first rolled by (3, -2) px), one stream, one
workspace per variant allocated up front.  HIP events around 5 calls, 9 alternating rounds (the order rotates from round to round), medians.
With --parent-lib <other libfav.so> (e.g. the parent commit's build) every variant runs on BOTH libraries, and before anything is timed the
outputs must be bit-identical and the workspace sizes equal: at 1280x720, at the ragged 150x203, and for fav_flow_pairs_rgb8_ex with
n_pairs = 6 (at 150x203).  The timing then gives, per variant, both medians and the parent's own noise (max - min) / median; a variant
passes when new median <= parent median x (1 + noise).
Without --step the script is the driver: each step below is a child process with a time limit of its own, and the first failure ends the
run.
usage: python scripts/flow_ab.py [--rounds 9] [--calls 5] [--parent-lib <other libfav.so>] > profiles/flow_ab.log"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"bits-150x203": 60, "pairs-150x203": 60, "time-1280x720": 240}      # step: its time limit in seconds (time: the bits first)
VARIANTS = {"bright": {}, "eps0.3": dict(smooth_eps=0.3), "grad": dict(data_term=1), "grad+eps0.3": dict(data_term=1, smooth_eps=0.3)}
MATCH_VARIANTS = {"match": dict(match_beta=-1), "match+grad+eps0.3": dict(match_beta=-1, data_term=1, smooth_eps=0.3)}      # this build only (_ex2)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--step", default="", choices=[""] + list(STEPS))
a = ap.parse_args()

if not a.step:
    for step, limit in STEPS.items():
        if step.startswith(("bits", "pairs")) and not a.parent_lib:
            continue
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + sys.argv[1:], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            sys.exit(f"flow_ab: step {step} failed ({rc}); nothing further is run")
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python"))
import torch
import fav_amd
from fav_amd import synth

dev = torch.device("cuda:0")
P, S = fav_amd._p, fav_amd._stream
libs = {"new": fav_amd.lib()}
if a.parent_lib:
    libs["parent"] = C.CDLL(os.path.abspath(a.parent_lib))
    libs["parent"].fav_last_error.restype = C.c_char_p
    for f in (libs["parent"].fav_flow_workspace_bytes_ex, libs["parent"].fav_flow_pairs_workspace_bytes_ex):
        f.restype = C.c_size_t
opts = {v: fav_amd._flow_opts_ex(o) for v, o in VARIANTS.items()}
opts.update({v: fav_amd._flow_opts_ex2(o) for v, o in MATCH_VARIANTS.items()})
EX = {v: "_ex" for v in VARIANTS}
EX.update({v: "_ex2" for v in MATCH_VARIANTS})
kind, size = a.step.split("-")
w, h = (int(x) for x in size.split("x"))
n = 6 if kind == "pairs" else 1
runs = [(v, l) for v in VARIANTS for l in libs] + [(v, "new") for v in MATCH_VARIANTS]

prev = [torch.from_numpy(synth.smooth_frame(h, w, 40 + k)).to(dev) for k in range(n)]
cur = [torch.roll(p, (-2, 3), (0, 1)).contiguous() for p in prev]
arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
nb, ws, out = {}, {}, {}
for v, l in runs:
    o = C.cast(C.pointer(opts[v]), C.c_void_p)
    nb[v, l] = getattr(libs[l], "fav_flow_pairs_workspace_bytes" + EX[v])(w, h, n, o) if kind == "pairs" else getattr(libs[l], "fav_flow_workspace_bytes" + EX[v])(w, h, o)
    assert nb[v, l] > 0, (v, l, libs[l].fav_last_error())
    ws[v, l] = torch.empty(nb[v, l], dtype=torch.uint8, device=dev)
    out[v, l] = [torch.empty((h, w, 2), dtype=torch.float32, device=dev) for _ in range(2 * n if kind == "pairs" else 1)]


def call(v, l):
    if kind == "pairs":
        rc = getattr(libs[l], "fav_flow_pairs_rgb8" + EX[v])(arr(prev), arr(cur), n, w, h, C.byref(opts[v]), arr(out[v, l][:n]), arr(out[v, l][n:]), P(ws[v, l]),
                                            C.c_size_t(nb[v, l]), S())
    else:
        rc = getattr(libs[l], "fav_flow_rgb8" + EX[v])(P(cur[0]), P(prev[0]), w, h, C.byref(opts[v]), P(out[v, l][0]), P(ws[v, l]), C.c_size_t(nb[v, l]), S())
    assert rc == 0, (v, l, rc, libs[l].fav_last_error())


for v, l in runs:                      # warm-up, and the bits
    call(v, l); call(v, l)
torch.cuda.synchronize()
for v in MATCH_VARIANTS:
    assert all(bool(torch.isfinite(t).all()) for t in out[v, "new"]), v
    print(f"{n} pair(s) of {w}x{h}, {v}: workspace {nb[v, 'new']} bytes, max |flow - bright's| "
          f"{max(float((x - y).abs().max()) for x, y in zip(out[v, 'new'], out['bright', 'new'])):.3f} px", flush=True)
for v in VARIANTS:
    assert all(bool(torch.isfinite(t).all()) for t in out[v, "new"]), v
    assert v == "bright" or not torch.equal(out[v, "new"][0], out["bright", "new"][0]), f"{v} computed the default variant"
    if "parent" in libs:
        assert nb[v, "new"] == nb[v, "parent"], (v, nb[v, "new"], nb[v, "parent"])
        assert all(torch.equal(x, y) for x, y in zip(out[v, "new"], out[v, "parent"])), f"{v}: the two builds differ at {w}x{h}"
        print(f"{n} pair(s) of {w}x{h}, {'both flows of each' if kind == 'pairs' else 'one flow'}, {v}: bit-identical to the parent build, "
              f"workspace {nb[v, 'new']} bytes on both", flush=True)
if kind != "time":
    sys.exit(0)

ms = {r: [] for r in runs}
for rnd in range(a.rounds):
    for r in runs[rnd % len(runs):] + runs[:rnd % len(runs)]:      # the order rotates: no run always follows the same one
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call(*r)
        e1.record(); e1.synchronize()
        ms[r].append(e0.elapsed_time(e1) / a.calls)
med = {r: statistics.median(ms[r]) for r in runs}
for v, l in runs:
    print(f"one pair of {w}x{h}, one flow, {v}, {l}: median {med[v, l]:.3f} ms (min {min(ms[v, l]):.3f}, max {max(ms[v, l]):.3f}, "
          f"{a.rounds} x {a.calls} calls, alternating; workspace {nb[v, l]} bytes)", flush=True)
print("  " + "; ".join(f"{v} / bright = {med[v, 'new'] / med['bright', 'new']:.3f}" for v in list(VARIANTS)[1:] + list(MATCH_VARIANTS)), flush=True)
# the prior's own launches at the level-1 size: the match of both directions (one launch), then the check of one
h1, w1 = (h + 1) // 2, (w + 1) // 2
g = [fav_amd.flow_down(fav_amd.flow_grey(t)) for t in (cur[0], prev[0])]
d_ab, d_ba = fav_amd.flow_match(g[0], g[1], 16)
stages = {"fav_flow_match_f32, R 16, both directions": lambda: fav_amd.flow_match(g[0], g[1], 16), "fav_flow_match_check": lambda: fav_amd.flow_match_check(d_ab, d_ba)}
for name, f in stages.items():
    f(); torch.cuda.synchronize()
    t = []
    for rnd in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            f()
        e1.record(); e1.synchronize()
        t.append(e0.elapsed_time(e1) / a.calls)
    print(f"  {name} at {w1}x{h1} (with the binding's two allocations): median {statistics.median(t):.3f} ms (min {min(t):.3f}, max {max(t):.3f})", flush=True)
if "parent" in libs:
    for v in VARIANTS:
        noise = (max(ms[v, "parent"]) - min(ms[v, "parent"])) / med[v, "parent"]
        ok = med[v, "new"] <= med[v, "parent"] * (1 + noise)
        print(f"  {v}: new / parent = {med[v, 'new'] / med[v, 'parent']:.4f}, the parent's own noise (max - min) / median = {noise:.4f}: "
              f"{'not slower' if ok else 'SLOWER beyond the noise'}", flush=True)
