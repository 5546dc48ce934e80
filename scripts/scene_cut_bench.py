#!/usr/bin/env python3
"""What -scene_cut costs and saves at 1280x720 ("Scene changes"; profiles/scene_cut_bench.log, profiles/scene_cut_cli.log).
  python scripts/scene_cut_bench.py op            fav_scene_change_rgb8 alone: time per pair with hipEvents around batches of back-to-back
                                                  calls, on noise, smooth and CONSTANT frames (the LDS-contention case), each checked
                                                  against the numpy model first
  python scripts/scene_cut_bench.py cli [frames]  fav_stylize -estimate_flow 1 on RAM-backed files, with and without -scene_cut 0.5, three
                                                  alternating rounds of one build: a clip without cuts, and one with a cut every 25 frames
Appends to $FAV_AB_OUT/scene_cut_bench.log / scene_cut_cli.log (default: build/, which git ignores)."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import numpy as np
from fav_amd import synth, t7
import scene_model as S

MODE = sys.argv[1] if len(sys.argv) > 1 else "op"
OUT = os.environ.get("FAV_AB_OUT") or os.path.join(ROOT, "build")
os.makedirs(OUT, exist_ok=True)
log = open(os.path.join(OUT, "scene_cut_bench.log" if MODE == "op" else "scene_cut_cli.log"), "a")
H, W = 720, 1280
HBM_TBS = 6.3            # achievable HBM read rate of the MI355X (DESIGN.md uses the same figure for the YCbCr kernels)


def say(s):
    print(s, flush=True); log.write(s + "\n"); log.flush()


def op():
    import torch
    import fav_amd
    dev = torch.device("cuda:0")

    def timed(fn, reps=500, warm=50, rounds=7):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record(); torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / reps)
        us.sort()
        return us[len(us) // 2], us[0], us[-1]

    floor_us = 2 * 3 * W * H / (HBM_TBS * 1e6)
    say(f"[op] library {os.path.relpath(fav_amd.LIB_PATH, ROOT)}; {W}x{H}; per pair: median (min .. max) over 7 rounds of 500 back-to-back calls, hipEvents; "
        f"one call = memset + 2 kernels; reading 2 x {3 * W * H / 1e6:.2f} MB at {HBM_TBS} TB/s takes {floor_us:.2f} us")
    rng = np.random.default_rng(1)
    const = lambda rgb: np.broadcast_to(np.array(rgb, np.uint8), (H, W, 3)).copy()
    inputs = [("noise", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)),
              ("smooth (blurred noise, sigma 8)", synth.smooth_frame(H, W, 1), synth.smooth_frame(H, W, 2)),
              ("constant, same colour (black)", const((0, 0, 0)), const((0, 0, 0))),
              ("constant, two colours", const((10, 200, 30)), const((250, 20, 90)))]
    ws = torch.empty(fav_amd.scene_change_workspace_bytes(), dtype=torch.uint8, device=dev)
    res = torch.empty(17, dtype=torch.int32, device=dev)
    for name, a, b in inputs:
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        got, want = fav_amd.scene_change(ta, tb, workspace=ws, result=res), S.scene_change(a, b)
        fn = lambda: fav_amd.lib().fav_scene_change_rgb8(fav_amd._p(ta), fav_amd._p(tb), W, H, fav_amd._p(ws), fav_amd.C.c_size_t(ws.numel()),
                                                         fav_amd._p(res), fav_amd._stream())
        m, lo, hi = timed(fn)
        say(f"[op] {name:34s} {m:7.2f} us  ({lo:.2f} .. {hi:.2f})   {floor_us / m * 100:5.1f} % of the HBM read rate   "
            f"equals the model: {got == want}   score {want[0] / (2.0 * W * H):.4f}")
    # the yardstick of the same session: the YCbCr conversion of one frame (about the same bytes)
    cf = fav_amd.yuv_format(0, 0, 1, 0)
    n = fav_amd.yuv_frame_bytes(W, H, cf)
    src, rgb = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev), torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    m, lo, hi = timed(lambda: fav_amd.yuv_to_rgb8(src, W, H, cf, out=rgb))
    say(f"[op] yardstick fav_yuv_to_rgb8 (420 centre), one frame, one kernel   {m:7.2f} us  ({lo:.2f} .. {hi:.2f})")


def cli():
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    exe = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize")
    d = tempfile.mkdtemp(prefix="fav_scene_cut_", dir="/dev/shm")
    vid, img = d + "/video.t7", d + "/image.t7"
    t7.make_synthetic_checkpoint(vid, seed=1234); t7.make_synthetic_checkpoint(img, arch=t7.IMAGE_ARCH, seed=1234, in_channels=3)
    # two smooth textures, 8 columns wider than the frame: a scene is a window that moves 1 px per frame, forth and back
    # (scene 0 bright, 128..247; scene 1 dark, 0..89: their luma bins are disjoint, the score across a cut is 1)
    tex = [(128 + synth.smooth_frame(H, W + 8, 1).astype(np.float32) * 0.47).astype(np.uint8),
           (synth.smooth_frame(H, W + 8, 2).astype(np.float32) * 0.35).astype(np.uint8)]
    os.makedirs(d + "/src")
    for s in range(2):
        for k in range(8):
            S.write_ppm(f"{d}/src/s{s}_{k}.ppm", np.ascontiguousarray(tex[s][:, k:k + W]))
    t_old = time.time() - 30.0            # finished inputs (host/fav_poll.h: anything younger than -poll_settle is watched first)
    for f in os.listdir(d + "/src"):
        os.utime(f"{d}/src/{f}", (t_old, t_old))
    pingpong = [0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1]
    clips = {"no cuts": lambda i: 0, "a cut every 25 frames": lambda i: ((i - 1) // 25) % 2}
    for cname, scene_of in clips.items():
        cd = f"{d}/{'cuts' if 'every' in cname else 'plain'}"
        os.makedirs(cd)
        for i in range(1, n + 1):
            os.symlink(f"{d}/src/s{scene_of(i)}_{pingpong[i % len(pingpong)]}.ppm", f"{cd}/frame_{i:05d}.ppm")
        fps = {"off": [], "-scene_cut 0.5": []}
        cuts = None
        for r in range(3):
            for name in fps:
                out = f"{d}/o"
                extra = ["-scene_cut", "0.5", "-scene_cut_log", out + "/log.txt"] if name != "off" else []
                res = subprocess.run([exe, "-input_pattern", cd + "/frame_%05d.ppm", "-estimate_flow", "1", "-model_vid", vid, "-model_img", img, "-gpu", "0",
                                      "-timing", "1", "-output_prefix", out + "/out"] + extra, capture_output=True, text=True)
                line = [l for l in res.stdout.splitlines() if l.startswith("{") and "fps_end_to_end" in l]
                if res.returncode or not line:
                    say(f"[cli] {cname} / {name}: FAILED {res.stderr[-400:]}"); sys.exit(1)
                j = json.loads(line[-1]); fps[name].append(j["fps_end_to_end"])
                say(f"[cli] {cname} / {name} round {r}: {line[-1]}")
                assert len([f for f in os.listdir(out) if f.endswith(".png")]) == n
                if extra:
                    cuts = sum(int(l.split()[3]) for l in open(out + "/log.txt"))
                shutil.rmtree(out, ignore_errors=True)
        for name, v in fps.items():
            say(f"[cli] {cname:22s} {name:15s} frames/s ({n} frames, {W}x{H}, three rounds): {' '.join('%.1f' % x for x in v)}"
                + (f"   cuts found: {cuts}" if name != "off" else ""))
    shutil.rmtree(d, ignore_errors=True)


if MODE == "op":
    op()
elif MODE == "cli":
    cli()
else:
    sys.exit(__doc__)
