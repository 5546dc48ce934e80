"""In-HBM rate of frames WITHOUT a prior (-create_inconsistent: every frame is a fav_stream_first_frame) at a given frame size, with and
without -scale_factor: canonical architecture, synthetic weights, the frame already on the device, PNG encode on the device included.
One JSON line.  FAV_AMD_LIB selects the library build (the unscaled leg needs nothing of this feature).
  python scripts/scale_bench.py --size 2160x3840 --factor 0.5 [--frames 40] [--warmup 5]
Kernel times: rocprofv3 --kernel-trace --stats -- python scripts/scale_bench.py ... (scale_prep_kernel, scale_planar_kernel)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python"))
import numpy as np
import torch
import fav_amd
from fav_amd import synth, t7

ap = argparse.ArgumentParser()
ap.add_argument("--size", default="2160x3840"); ap.add_argument("--factor", type=float, default=1.0)
ap.add_argument("--frames", type=int, default=40); ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()
h, w = (int(v) for v in a.size.split("x"))
dev = torch.device("cuda:0")
with tempfile.TemporaryDirectory() as d:
    ck = os.path.join(d, "m.t7"); t7.make_synthetic_checkpoint(ck, seed=1234)
    net = fav_amd.Net(ck, 0)
    first = t7.extract_layers(t7.load(ck)["model"])[0]
    pad = first["l"] if first["type"] == "pad" else 0        # the reflection padding folded into the network input
st = fav_amd.Stream(net, h, w)
hs, ws = h, w
if a.factor != 1.0:
    hs, ws = h * a.factor, w * a.factor
    assert hs == int(hs) and ws == int(ws), (hs, ws)
    hs, ws = int(hs), int(ws)
    st.set_single_image_size(hs, ws)
frames = [torch.from_numpy(synth.smooth_frame(h, w, 7 + k)).to(dev) for k in range(2)]
png, nbytes = st.png_buffers()


def run(n):
    for k in range(n):
        st.first_frame(frames[k & 1], want_f32=False)
        st.encode_png_into(png, nbytes)
    torch.cuda.synchronize()


run(a.warmup)
t0 = time.perf_counter(); run(a.frames); dt = time.perf_counter() - t0
net.check()
px_s, px_d = hs * ws, h * w
print(json.dumps({"size": [h, w], "factor": a.factor, "network_size": [hs, ws], "frames": a.frames, "ms_per_frame": round(1e3 * dt / a.frames, 3),
                  "frames_per_s": round(a.frames / dt, 2), "library": os.path.basename(fav_amd.LIB_PATH), "lib_path": fav_amd.LIB_PATH,
                  # minimum HBM traffic of the two resampling kernels (each byte once): u8 frame in + padded NHWC8 out; planar fp32 in + out
                  "scale_prep_min_bytes": 3 * px_d + 32 * (hs + 2 * pad) * (ws + 2 * pad) if a.factor != 1.0 else 0,
                  "scale_planar_min_bytes": 12 * px_s + 12 * px_d if a.factor != 1.0 else 0}))
