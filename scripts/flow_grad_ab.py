"""A/B of the estimator's gradient-constancy data term (fav_flow_opts_ex.data_term) on one 1280x720 pair, on one GPU, in one process:
  bright       fav_flow_rgb8 with default options (the brightness term through the entry of before)
  grad         fav_flow_rgb8_ex with data_term 1 (alpha 8): the five-plane coefficients with their 13-point warp stencil, the tensor sweeps
  grad+eps0.3  the same with smooth_eps 0.3: the weighted tensor sweeps
  parent       (with --parent-lib) default options on ANOTHER build of libfav.so, e.g. the parent commit's: what `bright` must not be slower than
synth.smooth_frame inputs (the second image is the first rolled by (3, -2) px), one stream, one workspace per variant allocated up front.
HIP events around 5 calls, 9 alternating rounds (the order rotates from round to round), medians -- the method of
scripts/flow_robust_ab.py.  bright and parent are compared bit for bit before anything is timed.
usage: python scripts/flow_grad_ab.py [--rounds 9] [--calls 5] [--parent-lib <other libfav.so>] > profiles/flow_grad_ab.log"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python"))
import torch
import fav_amd
from fav_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--parent-lib", default="")
ap.add_argument("--size", default="1280x720")
a = ap.parse_args()
dev = torch.device("cuda:0")
L, P, S = fav_amd.lib(), fav_amd._p, fav_amd._stream
w, h = (int(v) for v in a.size.split("x"))

prev = torch.from_numpy(synth.smooth_frame(h, w, 40)).to(dev)
cur = torch.roll(prev, (-2, 3), (0, 1)).contiguous()
variants = {"grad": dict(data_term=1), "grad+eps0.3": dict(data_term=1, smooth_eps=0.3)}
opts = {"bright": None, **{v: fav_amd._flow_opts_ex(o) for v, o in variants.items()}}
nb = {"bright": fav_amd.flow_workspace_bytes(w, h), **{v: fav_amd.flow_workspace_bytes(w, h, **o) for v, o in variants.items()}}
libs = {v: L for v in opts}
if a.parent_lib:
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    parent.fav_last_error.restype = C.c_char_p
    libs["parent"], opts["parent"], nb["parent"] = parent, None, nb["bright"]      # (default options: NULL)
ws = {v: torch.empty(nb[v], dtype=torch.uint8, device=dev) for v in libs}
out = {v: torch.empty((h, w, 2), dtype=torch.float32, device=dev) for v in libs}


def call(v):
    if v in variants:
        rc = libs[v].fav_flow_rgb8_ex(P(cur), P(prev), w, h, C.byref(opts[v]), P(out[v]), P(ws[v]), C.c_size_t(nb[v]), S())
    else:
        rc = libs[v].fav_flow_rgb8(P(cur), P(prev), w, h, None, P(out[v]), P(ws[v]), C.c_size_t(nb[v]), S())
    assert rc == 0, (v, rc, libs[v].fav_last_error())


for v in libs:                      # warm-up, and the bits
    call(v); call(v)
torch.cuda.synchronize()
if "parent" in libs:
    assert torch.equal(out["bright"], out["parent"]), "the brightness term and the other build differ"
for v in variants:
    assert not torch.equal(out["bright"], out[v]) and bool(torch.isfinite(out[v]).all()), v
ms = {v: [] for v in libs}
order = list(libs)
for rnd in range(a.rounds):
    for v in order[rnd % len(order):] + order[:rnd % len(order)]:      # the order rotates: no variant always follows the same one
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call(v)
        e1.record(); e1.synchronize()
        ms[v].append(e0.elapsed_time(e1) / a.calls)
for v in libs:
    m = statistics.median(ms[v])
    print(f"one pair of {w}x{h}, one flow, {v}: median {m:.3f} ms (min {min(ms[v]):.3f}, max {max(ms[v]):.3f}, {a.rounds} x {a.calls} calls, alternating; "
          f"workspace {nb[v]} bytes)", flush=True)
med = {v: statistics.median(ms[v]) for v in libs}
print(f"  grad / bright = {med['grad'] / med['bright']:.3f}; grad+eps0.3 / bright = {med['grad+eps0.3'] / med['bright']:.3f}"
      + (f"; bright / parent = {med['bright'] / med['parent']:.3f}, outputs bit-identical" if "parent" in libs else ""), flush=True)
