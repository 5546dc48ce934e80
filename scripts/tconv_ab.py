"""A/B of the transposed-convolution kernel (kernels_tconv.hip) on the canonical IMAGE architecture (t7.IMAGE_ARCH: ...,u64,u32,c9s1-3) at
1280x720: per-convolution times through fav_net_profile_read_host and the whole forward, alternating configurations in fresh child
processes (the kernel-selection switches are read once per process):
    tconv     libfav_diag.so as built                      (u64 / u32 on CK_TCONV, profile id 800 + N)
    stuffed   libfav_diag.so with FAV_NO_TCONV=1            (the generic kernel over the zero-stuffed input: what ran before)
    <name>    any other build of the library, --lib name=path (e.g. the parent commit's libfav.so)
Prints one JSON line per run and a summary; outputs of all configurations are compared with the first one's.
    python scripts/tconv_ab.py [--rounds 3] [--iters 100] [--lib parent=/path/to/libfav.so]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fast-artistic-videos_amd")
sys.path.insert(0, os.path.join(PKG, "python"))
FP32_MFMA_PEAK_TFLOPS = 157.3
H, W = 720, 1280


def child(ckpt, iters, out_npy):
    import time
    import numpy as np
    import torch
    import fav_amd
    net = fav_amd.Net(ckpt, 0)
    x = torch.from_numpy((np.random.default_rng(1).standard_normal((3, H, W)) * 50).astype(np.float32)).cuda()
    for _ in range(10): y = net.forward(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters): y = net.forward(x)
    torch.cuda.synchronize()
    fwd_ms = (time.perf_counter() - t0) * 1e3 / iters
    net.profile_enable(True)
    for _ in range(iters): net.forward(x)
    torch.cuda.synchronize()
    prof = net.profile_read()
    np.save(out_npy, y.cpu().numpy())
    print(json.dumps({"forward_ms": round(fwd_ms, 4), "conv_us": [round(ms / n * 1e3, 2) for (ms, n, macs, kid) in prof], "ids": [kid for (ms, n, macs, kid) in prof]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--lib", action="append", default=[]); ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.iters, a.child[1])
    import numpy as np
    from fav_amd import t7
    diag = os.path.join(PKG, "libfav_diag.so")
    configs = [("tconv", diag, {}), ("stuffed", diag, {"FAV_NO_TCONV": "1"})] + [(s.split("=", 1)[0], s.split("=", 1)[1], {}) for s in a.lib]
    d = tempfile.mkdtemp(prefix="tconv_ab")
    ckpt = os.path.join(d, "image.t7")
    t7.make_synthetic_checkpoint(ckpt, arch=t7.IMAGE_ARCH, seed=1234, in_channels=3)
    res = {name: [] for name, _, _ in configs}
    for r in range(a.rounds):
        for name, lib, env in configs:
            npy = os.path.join(d, name + ".npy")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--child", ckpt, npy],
                                 env=dict(os.environ, FAV_AMD_LIB=lib, **env), check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
            j = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            res[name].append(j)
            print(json.dumps(dict(j, config=name, round=r)), flush=True)
    # the two transposed layers are convolutions 13 and 14 of c9s1-32,d64,d128,R128 x 5,u64,u32,c9s1-3
    macs = {13: 360 * 640 * 64 * 128 * 9 / 4, 14: 720 * 1280 * 32 * 64 * 9 / 4}
    first = np.load(os.path.join(d, configs[0][0] + ".npy"))
    for name, _, _ in configs:
        fw = [j["forward_ms"] for j in res[name]]
        line = "%-8s forward ms %s" % (name, " ".join("%.3f" % v for v in fw))
        for li, m in macs.items():
            us = [j["conv_us"][li] for j in res[name]]
            line += " | conv%d (id %d) us %s, %.1f %% of the fp32 MFMA peak (useful MACs, best run)" % (
                li, res[name][0]["ids"][li], " ".join("%.1f" % v for v in us), 100 * 2 * m / (min(us) * 1e-6) / 1e12 / FP32_MFMA_PEAK_TFLOPS)
        line += " | max |out - %s| %.3e (150*tanh units)" % (configs[0][0], float(np.abs(np.load(os.path.join(d, name + ".npy")) - first).max()))
        print(line)


if __name__ == "__main__":
    main()
