"""360 degrees from equirectangular frames, measured on one GPU.
  leg 1: the transform kernel alone (fav_vr_equi_to_faces_rgb8), 2560x1440 -> 6 x 768^2 (overlap 128) and 6 x 1504^2 (overlap 250),
         supersample 1, 2 and 4: HIP events around --calls calls, --rounds alternating rounds, medians (the method of flow_pairs_ab.py)
  leg 2: end to end at 6 x 768^2, canonical architecture with synthetic weights, --frames frames of 2560x1440: `-timing 1` frames/s of
         fav_stylize_vr -input_equi_pattern against the file route (faces from fav_transform_vr, flows from fav_flow -batch, all on disk
         before the timed run starts) on the same clip, two alternating runs each; the PNG files of the two routes are compared.
usage: python scripts/equi_bench.py [--rounds 9] [--calls 20] [--frames 6] [--skip-e2e] > profiles/equi_bench.log"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import numpy as np
import torch
import fav_amd
from fav_amd import t7
import equi_model as E

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--frames", type=int, default=6)
ap.add_argument("--skip-e2e", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
EW, EH = 2560, 1440
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")


def textured(n):
    """the sphere function turned by 0.01 rad per frame, plus a fixed fine texture turning with it (so PNG sizes are those of a picture)"""
    img = E.sphere_image(EW, EH, 0.01 * n).astype(np.int16)
    tex = (np.random.default_rng(7).integers(-12, 13, (EH // 4, EW // 4, 3))).repeat(4, 0).repeat(4, 1)
    return np.clip(img + np.roll(tex, 3 * n, axis=1), 0, 255).astype(np.uint8)


def kernel_leg(edge, ov):
    src = torch.from_numpy(textured(0)).to(dev)
    variants = (1, 2, 4)
    for s in variants:
        fav_amd.vr_equi_to_faces(src, edge, ov, supersample=s)
    torch.cuda.synchronize()
    faces = [torch.empty((edge, edge, 3), dtype=torch.uint8, device=dev) for _ in range(6)]
    import ctypes as C
    arr = (C.c_void_p * 6)(*[t.data_ptr() for t in faces])
    L, P, S = fav_amd.lib(), fav_amd._p, fav_amd._stream
    ms = {s: [] for s in variants}
    for _ in range(a.rounds):
        for s in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fav_amd._check(L.fav_vr_equi_to_faces_rgb8(P(src), EW, EH, edge, edge, ov, ov, s, arr, None, S()))
            e1.record(); e1.synchronize()
            ms[s].append(e0.elapsed_time(e1) / a.calls)
    for s in variants:
        m = statistics.median(ms[s])
        px = 6 * edge * edge
        print(f"transform {EW}x{EH} -> 6 x {edge}^2, overlap {ov}, supersample {s}: median {m * 1e3:.1f} us (min {min(ms[s]) * 1e3:.1f}, max {max(ms[s]) * 1e3:.1f}; "
              f"{a.rounds} x {a.calls} calls, alternating); {px / m / 1e6:.2f} Gpixel/s out, {48 * s * s * px / m / 1e9:.2f} T taps/s, "
              f"{(3 * EW * EH + 3 * px) / m / 1e6:.1f} GB/s of compulsory traffic", flush=True)


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"{cmd}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def e2e_leg(edge, ov):
    with tempfile.TemporaryDirectory() as d:
        ck = os.path.join(d, "m.t7"); t7.make_synthetic_checkpoint(ck, arch=t7.CANONICAL_ARCH, seed=1)
        for n in range(a.frames):
            E.write_ppm(os.path.join(d, f"frame_{n + 1:05d}.ppm"), textured(n))
        geom = ["-overlap_pixel_w", str(ov), "-overlap_pixel_h", str(ov)]
        run([os.path.join(BIN, "fav_transform_vr"), "-input_equi_pattern", os.path.join(d, "frame_%05d.ppm"), "-output_pattern", os.path.join(d, "faces", "frame_%05d-%d.ppm"),
             "-cube_edge_length", str(edge)] + geom)
        lines = []
        for face in E.PROC_ORDER:
            os.makedirs(os.path.join(d, f"flow-{face}"))
            for fr in range(2, a.frames + 1):
                cur, prev = (os.path.join(d, "faces", f"frame_{k:05d}-{face}.ppm") for k in (fr, fr - 1))
                lines += [f"{cur} {prev} {d}/flow-{face}/backward_{fr}_{fr - 1}.flo", f"{prev} {cur} {d}/flow-{face}/forward_{fr - 1}_{fr}.flo"]
        open(os.path.join(d, "list.txt"), "w").write("\n".join(lines) + "\n")
        run([os.path.join(BIN, "fav_flow"), "-batch", os.path.join(d, "list.txt")])
        common = ["-model_vid", ck, "-model_img", "self", "-gpu", "0", "-out_equi", "-out_equi_w", str(EW), "-out_equi_h", str(EH), "-out_cubemap", "-timing", "1",
                  "-poll_settle", "0"] + geom
        routes = {"files": ["-input_pattern", os.path.join(d, "faces", "frame_%05d-%d.ppm"), "-flow_pattern", os.path.join(d, "flow-%d", "backward_[%d]_{%d}.flo"),
                            "-forward_flow_pattern", os.path.join(d, "flow-%d", "forward_{%d}_[%d].flo")],
                  "equi": ["-input_equi_pattern", os.path.join(d, "frame_%05d.ppm"), "-cube_edge_length", str(edge)]}
        fps = {k: [] for k in routes}
        for rnd in range(2):
            for k, args in routes.items():
                out = run([os.path.join(BIN, "fav_stylize_vr")] + args + common + ["-output_prefix", os.path.join(d, k, "out")])
                fps[k].append(float(re.search(r"frames \(x6 faces\) in [0-9.]+ s: ([0-9.]+) frames/s", out).group(1)))
        same = all(open(os.path.join(d, "files", nm), "rb").read() == open(os.path.join(d, "equi", nm), "rb").read() for nm in sorted(os.listdir(os.path.join(d, "files"))))
        what = {"files": "file route (18 files per frame read: 6 faces, 12 flows; transform and flows made beforehand, not timed)",
                "equi": "-input_equi_pattern (1 file per frame read; transform and 12 flows inside the timed loop)"}
        for k in routes:
            print(f"end to end, {a.frames} frames of {EW}x{EH} -> 6 x {edge}^2, overlap {ov}, canonical architecture, -structure 1, equi {EW}x{EH} + cube map PNGs, "
                  f"{what[k]}: {' / '.join('%.2f' % f for f in fps[k])} frames/s (-timing 1, two runs, alternating)", flush=True)
        print(f"  PNG files of the two routes byte-equal: {same}", flush=True)


kernel_leg(768, 128)
kernel_leg(1504, 250)
if not a.skip_e2e:
    e2e_leg(768, 128)
