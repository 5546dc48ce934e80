"""A/B of the estimator's median filter (fav_flow_opts_ex3.median) on one 1280x720 pair, on one GPU, by the method of scripts/flow_ab.py:
  off       default options through fav_flow_rgb8_ex3 with median 0
  median3   the 3 x 3 filter after every warp
  median5   the 5 x 5 filter
and, with --parent-lib <other libfav.so> (the parent commit's build, which has no _ex3 entries),
  parent    default options through the parent's fav_flow_rgb8_ex2
whose flow must be bit-identical to `off` and whose workspace must have the size of all three before anything is timed.
synth.smooth_frame inputs (the second image is the first rolled by (3, -2) px), one stream, one workspace per run allocated up front.  HIP
events around 5 calls, 9 alternating rounds (the order rotates from round to round), medians.  `off` passes when its median <= the
parent's median x (1 + the parent's own noise (max - min) / median).  Then the same for the batched call on six pairs of 1280x720
(fav_flow_pairs_rgb8_ex3 | the parent's _ex2), and the filter alone (fav_flow_median_f32) at 1280x720.
Without --step the script is the driver: each step is a child process with a time limit of its own, and the first failure ends the run.
usage: python scripts/flow_median_ab.py [--rounds 9] [--calls 5] [--parent-lib <other libfav.so>] > profiles/flow_median_ab.log"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"single": 240, "pairs": 240}      # step: its time limit in seconds
W, H = 1280, 720

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--step", default="", choices=[""] + list(STEPS))
a = ap.parse_args()

if not a.step:
    for step, limit in STEPS.items():
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + sys.argv[1:], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            sys.exit(f"flow_median_ab: step {step} failed ({rc}); nothing further is run")
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python"))
import torch
import fav_amd
from fav_amd import synth

dev = torch.device("cuda:0")
P, S = fav_amd._p, fav_amd._stream
new = fav_amd.lib()
n = 6 if a.step == "pairs" else 1
runs = {"off": (new, "_ex3", fav_amd._flow_opts_ex3({})), "median3": (new, "_ex3", fav_amd._flow_opts_ex3(dict(median=3))),
        "median5": (new, "_ex3", fav_amd._flow_opts_ex3(dict(median=5)))}
if a.parent_lib:
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    parent.fav_last_error.restype = C.c_char_p
    parent.fav_flow_workspace_bytes_ex2.restype = C.c_size_t
    parent.fav_flow_pairs_workspace_bytes_ex2.restype = C.c_size_t
    assert not hasattr(parent, "fav_flow_rgb8_ex3"), "--parent-lib has the _ex3 entries: it is not the parent commit's build"
    runs["parent"] = (parent, "_ex2", fav_amd._flow_opts_ex2({}))

prev = [torch.from_numpy(synth.smooth_frame(H, W, 40 + k)).to(dev) for k in range(n)]
cur = [torch.roll(p, (-2, 3), (0, 1)).contiguous() for p in prev]
arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
nb, ws, out = {}, {}, {}
for r, (lib, ex, o) in runs.items():
    ov = C.cast(C.pointer(o), C.c_void_p)
    nb[r] = getattr(lib, "fav_flow_pairs_workspace_bytes" + ex)(W, H, n, ov) if a.step == "pairs" else getattr(lib, "fav_flow_workspace_bytes" + ex)(W, H, ov)
    assert nb[r] > 0, (r, lib.fav_last_error())
    ws[r] = torch.empty(nb[r], dtype=torch.uint8, device=dev)
    out[r] = [torch.empty((H, W, 2), dtype=torch.float32, device=dev) for _ in range(2 * n if a.step == "pairs" else 1)]
assert len(set(nb.values())) == 1, nb      # the filter owns no part of the workspace


def call(r):
    lib, ex, o = runs[r]
    if a.step == "pairs":
        rc = getattr(lib, "fav_flow_pairs_rgb8" + ex)(arr(prev), arr(cur), n, W, H, C.byref(o), arr(out[r][:n]), arr(out[r][n:]), P(ws[r]), C.c_size_t(nb[r]), S())
    else:
        rc = getattr(lib, "fav_flow_rgb8" + ex)(P(cur[0]), P(prev[0]), W, H, C.byref(o), P(out[r][0]), P(ws[r]), C.c_size_t(nb[r]), S())
    assert rc == 0, (r, rc, lib.fav_last_error())


what = f"{n} pair(s) of {W}x{H}, {'both flows of each' if a.step == 'pairs' else 'one flow'}"
for r in runs:                      # warm-up, and the bits
    call(r); call(r)
torch.cuda.synchronize()
for r in runs:
    assert all(bool(torch.isfinite(t).all()) for t in out[r]), r
for r in ("median3", "median5"):
    assert not torch.equal(out[r][0], out["off"][0]), f"{r} computed the unfiltered flow"
    print(f"{what}, {r}: workspace {nb[r]} bytes (as off), max |flow - off's| {max(float((x - y).abs().max()) for x, y in zip(out[r], out['off'])):.3f} px", flush=True)
if "parent" in runs:
    assert all(torch.equal(x, y) for x, y in zip(out["off"], out["parent"])), "median 0 and the parent build differ"
    print(f"{what}, off: bit-identical to the parent build, workspace {nb['off']} bytes on both", flush=True)

ms = {r: [] for r in runs}
order = list(runs)
for rnd in range(a.rounds):
    for r in order[rnd % len(order):] + order[:rnd % len(order)]:      # the order rotates: no run always follows the same one
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call(r)
        e1.record(); e1.synchronize()
        ms[r].append(e0.elapsed_time(e1) / a.calls)
med = {r: statistics.median(ms[r]) for r in runs}
for r in runs:
    print(f"{what}, {r}: median {med[r]:.3f} ms per call (min {min(ms[r]):.3f}, max {max(ms[r]):.3f}, {a.rounds} x {a.calls} calls, alternating)", flush=True)
print("  " + "; ".join(f"{r} / off = {med[r] / med['off']:.3f} (+{(med[r] - med['off']) * 1000:.0f} us)" for r in ("median3", "median5")), flush=True)
if "parent" in runs:
    noise = (max(ms["parent"]) - min(ms["parent"])) / med["parent"]
    ok = med["off"] <= med["parent"] * (1 + noise)
    print(f"  off / parent = {med['off'] / med['parent']:.4f}, the parent's own noise (max - min) / median = {noise:.4f}: {'not slower' if ok else 'SLOWER beyond the noise'}", flush=True)
if a.step == "single":      # the filter alone, into a buffer allocated up front
    f_in, f_out = out["off"][0], torch.empty_like(out["off"][0])
    for size in (3, 5):
        t = []
        for rnd in range(a.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                assert new.fav_flow_median_f32(P(f_in), P(f_out), W, H, size, S()) == 0
            e1.record(); e1.synchronize()
            if rnd:
                t.append(e0.elapsed_time(e1) / a.calls)
        print(f"  fav_flow_median_f32 at {W}x{H}, size {size}: median {statistics.median(t) * 1000:.1f} us (min {min(t) * 1000:.1f}, max {max(t) * 1000:.1f}); "
              f"{W * H * 16 / statistics.median(t) / 1e9:.2f} TB/s of the 16 bytes per pixel it moves", flush=True)
