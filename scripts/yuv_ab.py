"""Kernel times of the Y4M route at 1280x720 beside the PNG encoder's, with hipEvents (profiles/yuv_ab.log; DESIGN.md, "Y4M in and out").
  python scripts/yuv_ab.py new               this tree's library: fav_stream_encode_png, fav_stream_encode_yuv, the three operators
  python scripts/yuv_ab.py parent <dir>      a built checkout of the parent commit in <dir> (its library and binding): the PNG encode only
Appends to $FAV_AB_OUT/yuv_ab.log (default: build/yuv_ab.log, which git ignores)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = sys.argv[1]
if MODE == "parent":
    os.environ["FAV_AMD_LIB"] = os.path.join(sys.argv[2], "fast-artistic-videos_amd", "libfav.so")
    sys.path.insert(0, os.path.join(sys.argv[2], "fast-artistic-videos_amd", "python"))
else:
    sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import numpy as np
import torch
import fav_amd
from fav_amd import synth, t7

OUT = os.environ.get("FAV_AB_OUT") or os.path.join(ROOT, "build")
os.makedirs(OUT, exist_ok=True)
log = open(os.path.join(OUT, "yuv_ab.log"), "a")


def say(s):
    print(s); log.write(s + "\n"); log.flush()


def timed(fn, reps=200, warm=20, rounds=7):
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


H, W = 720, 1280
dev = torch.device("cuda:0")
ck = os.path.join(OUT, "synthetic_model.t7")
if not os.path.exists(ck):
    t7.make_synthetic_checkpoint(ck, seed=1)
net = fav_amd.Net(ck, 0)
st = fav_amd.Stream(net, H, W)
st.first_frame(torch.from_numpy(synth.smooth_frame(H, W, 1)).to(dev))
torch.cuda.synchronize()
say(f"[{MODE}] library {fav_amd.LIB_PATH}; {W}x{H}; per call: median (min .. max) over 7 rounds of 200 back-to-back calls, hipEvents")
png, nb = st.png_buffers()
m, lo, hi = timed(lambda: st.encode_png_into(png, nb))
say(f"[{MODE}] fav_stream_encode_png            {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   file {int(nb.item())} bytes")
if MODE == "new":
    import yuv_model as M
    px = H * W
    for name, cf, f in (("420 centre, BT.709, limited", fav_amd.yuv_format(0, 0, 1, 0), M.Format("420", "center", "709", False)),
                        ("444, BT.709, limited", fav_amd.yuv_format(1, 0, 1, 0), M.Format("444", "center", "709", False))):
        n = fav_amd.yuv_frame_bytes(W, H, cf)
        buf = torch.empty(n, dtype=torch.uint8, device=dev)
        m, lo, hi = timed(lambda: st.encode_yuv_into(buf, cf))
        byts = 12 * px + n
        say(f"[new] fav_stream_encode_yuv ({name})  {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   {byts / 1e6:.2f} MB moved -> {byts / m / 1e6:.2f} TB/s (the 11 MB state stays in the Infinity Cache between calls)")
        # same bytes as the model (the state's 8-bit image through the model)
        state = st.state().cpu().numpy()
        want = M.rgb_f32_to_yuv(state, f)
        say(f"[new]   equals the fp32 model at 1280x720: {bool(np.array_equal(buf.cpu().numpy(), want))}")
        # cold: 32 distinct fp32 images (354 MB, more than the 256 MiB Infinity Cache) in turn
        imgs = [torch.rand(3, H, W, device=dev) for _ in range(32)]
        k = [0]
        def cold():
            fav_amd.rgb_to_yuv(imgs[k[0] % 32], cf, out=buf); k[0] += 1
        m, lo, hi = timed(cold, reps=192)
        say(f"[new] fav_rgb_f32_to_yuv ({name}), 32 images in turn (354 MB)  {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   {byts / m / 1e6:.2f} TB/s = {100 * byts / m / 1e6 / 8.0:.0f} % of the 8 TB/s peak, {100 * byts / m / 1e6 / 6.3:.0f} % of the 6.3 TB/s achievable")
        del imgs
        rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        src = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev)
        m, lo, hi = timed(lambda: fav_amd.yuv_to_rgb8(src, W, H, cf, out=rgb))
        byts = n + 3 * px
        say(f"[new] fav_yuv_to_rgb8 ({name})        {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   {byts / 1e6:.2f} MB moved -> {byts / m / 1e6:.2f} TB/s (cache-resident)")
        srcs = [torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev) for _ in range(64)]
        rgbs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(64)]
        def cold_dec():
            fav_amd.yuv_to_rgb8(srcs[k[0] % 64], W, H, cf, out=rgbs[k[0] % 64]); k[0] += 1
        m, lo, hi = timed(cold_dec, reps=192)
        say(f"[new] fav_yuv_to_rgb8 ({name}), 64 frames in turn ({64 * byts / 1e6:.0f} MB)  {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   {byts / m / 1e6:.2f} TB/s")
        del srcs, rgbs
        w8 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
        m, lo, hi = timed(lambda: fav_amd.rgb_to_yuv(w8, cf, out=buf))
        say(f"[new] fav_rgb8_to_yuv ({name})        {m:8.2f} us  ({lo:.2f} .. {hi:.2f})")
st.close(); net.close()
