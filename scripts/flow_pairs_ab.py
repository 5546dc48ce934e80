"""A/B of the batched bidirectional flow estimator against the loop of single-pair calls it replaces, on one GPU, in one process.
  leg 1: 6 pairs of 1504x1504 (the six cube faces of scripts/vr_bench.py): ONE fav_flow_pairs_rgb8 call against 12 fav_flow_rgb8 calls
  leg 2: 1 pair of 1280x720: the batch of one against the two single calls of fav_stream_next_frame_estimate
Default options, synth.smooth_frame inputs (the second image of a pair is the first rolled by (3, -2) px), one stream, one workspace per
variant allocated up front.  HIP events around 5 calls, 9 alternating rounds, medians -- the method of
profiles/flow_720p_sweeps_per_launch_ab.log.  Both variants' outputs are compared bit for bit before anything is timed.
usage: python scripts/flow_pairs_ab.py [--rounds 9] [--calls 5] > profiles/flow_pairs_ab.log"""
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
a = ap.parse_args()
dev = torch.device("cuda:0")
L, P, S = fav_amd.lib(), fav_amd._p, fav_amd._stream


def leg(n, h, w):
    prev = [torch.from_numpy(synth.smooth_frame(h, w, 40 + k)).to(dev) for k in range(n)]
    cur = [torch.roll(p, (-2, 3), (0, 1)).contiguous() for p in prev]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    nb1, nbn = fav_amd.flow_workspace_bytes(w, h), fav_amd.flow_pairs_workspace_bytes(w, h, n)
    ws1, wsn = torch.empty(nb1, dtype=torch.uint8, device=dev), torch.empty(nbn, dtype=torch.uint8, device=dev)
    out = {v: [torch.empty((h, w, 2), dtype=torch.float32, device=dev) for _ in range(2 * n)] for v in ("loop", "batch")}
    A = {"prev": arr(prev), "cur": arr(cur), "bw": arr(out["batch"][:n]), "fw": arr(out["batch"][n:])}

    def loop():
        for k in range(n):
            fav_amd._check(L.fav_flow_rgb8(P(cur[k]), P(prev[k]), w, h, None, P(out["loop"][k]), P(ws1), C.c_size_t(nb1), S()))
            fav_amd._check(L.fav_flow_rgb8(P(prev[k]), P(cur[k]), w, h, None, P(out["loop"][n + k]), P(ws1), C.c_size_t(nb1), S()))

    def batch():
        fav_amd._check(L.fav_flow_pairs_rgb8(A["prev"], A["cur"], n, w, h, None, A["bw"], A["fw"], P(wsn), C.c_size_t(nbn), S()))

    variants = {"loop": loop, "batch": batch}
    for f in variants.values():                      # warm-up, and the bits
        f(); f()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out["loop"], out["batch"])), "the batch and the loop differ"
    ms = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record(); e1.synchronize()
            ms[v].append(e0.elapsed_time(e1) / a.calls)
    what = {"loop": f"{2 * n} fav_flow_rgb8 calls", "batch": f"one fav_flow_pairs_rgb8 call, n_pairs {n}"}
    for v in variants:
        m = statistics.median(ms[v])
        print(f"{n} pair(s) of {w}x{h}, default options, {what[v]}: median {m:.3f} ms ({m / n:.3f} ms per pair = both directions, "
              f"{m / (2 * n):.3f} ms per flow; min {min(ms[v]):.3f}, max {max(ms[v]):.3f}, {a.rounds} x {a.calls} calls, alternating)", flush=True)
    print(f"  outputs bit-identical; loop / batch = {statistics.median(ms['loop']) / statistics.median(ms['batch']):.2f}; "
          f"workspace {nbn} bytes (batch) against {nb1} (loop)", flush=True)


leg(6, 1504, 1504)
leg(1, 720, 1280)
