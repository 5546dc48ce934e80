#!/usr/bin/env python3
"""File -> PNG frames/s of the CLI with -create_inconsistent (every frame without a prior, through the IMAGE model: the per-frame baseline
mode) and a `u<n>` image model (t7.IMAGE_ARCH) at 1280x720, on RAM-backed files, alternating builds of bin/fav_stylize:
    tconv_cli.py [frames] [name=path/to/fav_stylize ...]      (default: this tree's build only; each executable finds its libfav.so next to bin/)
Three rounds; prints the CLI's own timing line (-timing 1) per run and the frames/s of every run per build."""
import json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as O
from fav_amd import synth, t7
H, W = 720, 1280
N = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 200
builds = [("this", os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize"))] + [tuple(a.split("=", 1)) for a in sys.argv[1:] if "=" in a]
d = tempfile.mkdtemp(prefix="fav_tconv_cli_", dir="/dev/shm")
os.makedirs(d + "/src")
vid, img = d + "/video.t7", d + "/image.t7"
t7.make_synthetic_checkpoint(vid, seed=1234); t7.make_synthetic_checkpoint(img, arch=t7.IMAGE_ARCH, seed=1234, in_channels=3)
for k in range(4): O.write_pnm(f"{d}/src/f{k}.ppm", synth.random_frame(H, W, k))
t_old = time.time() - 30.0            # finished inputs (host/fav_poll.h: anything younger than -poll_settle is watched first)
for f in os.listdir(d + "/src"): os.utime(f"{d}/src/{f}", (t_old, t_old))
for i in range(1, N + 1): os.symlink(f"{d}/src/f{i % 4}.ppm", f"{d}/frame_{i:05d}.ppm")
fps = {name: [] for name, _ in builds}
for r in range(3):
    for name, exe in builds:
        out = f"{d}/o_{name}"
        res = subprocess.run([exe, "-input_pattern", d + "/frame_%05d.ppm", "-create_inconsistent", "-model_vid", vid, "-model_img", img, "-gpu", "0", "-timing", "1",
                              "-png_encoder", "gpu", "-output_prefix", out + "/out"], capture_output=True, text=True)
        line = [l for l in res.stdout.splitlines() if l.startswith("{") and "fps_end_to_end" in l]
        if not line: print(name, "FAILED", res.stderr[-400:]); sys.exit(1)
        j = json.loads(line[-1]); fps[name].append(j["fps_end_to_end"])
        print(name, "round", r, line[-1], flush=True)
        assert len([f for f in os.listdir(out) if f.endswith(".png")]) == N
        shutil.rmtree(out, ignore_errors=True)
for name, v in fps.items(): print("%-8s -create_inconsistent frames/s (%d frames, 1280x720): %s" % (name, N, " ".join("%.1f" % x for x in v)))
shutil.rmtree(d, ignore_errors=True)
