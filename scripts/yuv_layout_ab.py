"""Kernel times of the deep / 4:2:2 Y4M route at 1280x720 beside the 8-bit calls, with hipEvents (profiles/yuv_layout_ab.log; DESIGN.md,
"Y4M in and out").
  python scripts/yuv_layout_ab.py new             this tree's library: the 8-bit calls, then fav_stream_encode_yuv_layout (420p10, 422p10)
                                                  and fav_yuv_layout_to_rgb8 (420p10)
  python scripts/yuv_layout_ab.py parent <dir>    a built checkout of the parent commit in <dir> (its library and binding): the 8-bit calls
Run both in one session: the 8-bit calls of the two libraries are compared within the spread of their rounds.
Appends to $FAV_AB_OUT/yuv_layout_ab.log (default: build/yuv_layout_ab.log, which git ignores)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = sys.argv[1]
if MODE == "parent":
    os.environ["FAV_AMD_LIB"] = os.path.join(sys.argv[2], "fast-artistic-videos_amd", "libfav.so")
    sys.path.insert(0, os.path.join(sys.argv[2], "fast-artistic-videos_amd", "python"))
else:
    sys.path.insert(0, os.path.join(ROOT, "fast-artistic-videos_amd", "python"))
import torch
import fav_amd
from fav_amd import synth, t7

OUT = os.environ.get("FAV_AB_OUT") or os.path.join(ROOT, "build")
os.makedirs(OUT, exist_ok=True)
log = open(os.path.join(OUT, "yuv_layout_ab.log"), "a")


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


def line(name, t, moved):
    m, lo, hi = t
    say(f"[{MODE}] {name:58s} {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   {moved / 1e6:6.2f} MB moved -> {moved / m / 1e6:.2f} TB/s")


H, W = 720, 1280
px = H * W
dev = torch.device("cuda:0")
ck = os.path.join(OUT, "synthetic_model.t7")
if not os.path.exists(ck):
    t7.make_synthetic_checkpoint(ck, seed=1)
net = fav_amd.Net(ck, 0)
st = fav_amd.Stream(net, H, W)
st.first_frame(torch.from_numpy(synth.smooth_frame(H, W, 1)).to(dev))
torch.cuda.synchronize()
say(f"[{MODE}] library {fav_amd.LIB_PATH}; {W}x{H}, BT.709, limited; per call: median (min .. max) over 7 rounds of 200 back-to-back calls, "
    "hipEvents; buffers stay cache-resident between calls")
rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
# the 8-bit calls: the same in both libraries
cf = fav_amd.yuv_format(0, 0, 1, 0)
n8 = fav_amd.yuv_frame_bytes(W, H, cf)
buf8 = torch.empty(n8, dtype=torch.uint8, device=dev)
src8 = torch.randint(0, 256, (n8,), dtype=torch.uint8, device=dev)
line("fav_stream_encode_yuv (420jpeg)", timed(lambda: st.encode_yuv_into(buf8, cf)), 12 * px + n8)
line("fav_yuv_to_rgb8 (420jpeg)", timed(lambda: fav_amd.yuv_to_rgb8(src8, W, H, cf, out=rgb)), n8 + 3 * px)
if MODE == "new":
    for name, cl in (("420p10", fav_amd.yuv_layout(fav_amd.YUV_420, 0, 1, 0, 10)), ("422p10", fav_amd.yuv_layout(fav_amd.YUV_422, 1, 1, 0, 10)),
                     ("422, 8 bits", fav_amd.yuv_layout(fav_amd.YUV_422, 1, 1, 0, 8)), ("420jpeg through the layout entry", fav_amd.yuv_layout(0, 0, 1, 0, 8))):
        n = fav_amd.yuv_layout_frame_bytes(W, H, cl)
        buf = torch.empty(n, dtype=torch.uint8, device=dev)
        line(f"fav_stream_encode_yuv_layout ({name})", timed(lambda: st.encode_yuv_layout_into(buf, cl)), 12 * px + n)
    for name, cl in (("420p10", fav_amd.yuv_layout(fav_amd.YUV_420, 0, 1, 0, 10)), ("422p10", fav_amd.yuv_layout(fav_amd.YUV_422, 1, 1, 0, 10))):
        n = fav_amd.yuv_layout_frame_bytes(W, H, cl)
        src = (torch.randint(0, 1024, (n // 2,), dtype=torch.int32, device=dev).to(torch.int16)).view(torch.uint8)
        line(f"fav_yuv_layout_to_rgb8 ({name})", timed(lambda: fav_amd.yuv_layout_to_rgb8(src, W, H, cl, out=rgb)), n + 3 * px)
st.close(); net.close()
