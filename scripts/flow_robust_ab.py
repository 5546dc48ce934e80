"""A/B of the estimator's edge-preserving smoothness (fav_flow_opts.smooth_eps) on one 1280x720 pair, on one GPU, in one process:
  eps0    fav_flow_rgb8 with default options (smooth_eps 0: the quadratic term, the launches of before)
  eps0.3  the same call with smooth_eps 0.3 (alpha 5): the weighted sweeps and the 13-point weight stencil in the coefficient launch
  parent  (with --parent-lib) default options on ANOTHER build of libfav.so, e.g. the parent commit's: what eps0 must not be slower than
synth.smooth_frame inputs (the second image is the first rolled by (3, -2) px), one stream, one workspace per variant allocated up front.
HIP events around 5 calls, 9 alternating rounds (the order rotates from round to round), medians -- the method of
scripts/flow_pairs_ab.py.  eps0 and parent are compared bit for bit before anything is timed.
usage: python scripts/flow_robust_ab.py [--rounds 9] [--calls 5] [--parent-lib <other libfav.so>] > profiles/flow_robust_ab.log"""
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
opts = {"eps0": None, "eps0.3": fav_amd._flow_opts(dict(smooth_eps=0.3))}
nb = {"eps0": fav_amd.flow_workspace_bytes(w, h), "eps0.3": fav_amd.flow_workspace_bytes(w, h, smooth_eps=0.3)}
libs = {"eps0": L, "eps0.3": L}
if a.parent_lib:
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    parent.fav_last_error.restype = C.c_char_p
    libs["parent"], opts["parent"], nb["parent"] = parent, None, nb["eps0"]      # (default options: NULL, whatever the struct's size there)
ws = {v: torch.empty(nb[v], dtype=torch.uint8, device=dev) for v in libs}
out = {v: torch.empty((h, w, 2), dtype=torch.float32, device=dev) for v in libs}


def call(v):
    o = C.byref(opts[v]) if opts[v] is not None else None
    rc = libs[v].fav_flow_rgb8(P(cur), P(prev), w, h, o, P(out[v]), P(ws[v]), C.c_size_t(nb[v]), S())
    assert rc == 0, (v, rc, libs[v].fav_last_error())


for v in libs:                      # warm-up, and the bits
    call(v); call(v)
torch.cuda.synchronize()
if "parent" in libs:
    assert torch.equal(out["eps0"], out["parent"]), "smooth_eps 0 and the other build differ"
assert not torch.equal(out["eps0"], out["eps0.3"]) and bool(torch.isfinite(out["eps0.3"]).all())
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
print(f"  eps0.3 / eps0 = {statistics.median(ms['eps0.3']) / statistics.median(ms['eps0']):.3f}"
      + (f"; eps0 / parent = {statistics.median(ms['eps0']) / statistics.median(ms['parent']):.3f}, outputs bit-identical" if "parent" in libs else ""), flush=True)
