"""Call times of the -original_colors encodes at 1280x720 beside the plain ones, with hipEvents (profiles/color_ab.log; DESIGN.md,
"Original colours").
  python scripts/color_ab.py new               this tree's library: fav_stream_encode_yuv_colors against fav_stream_encode_yuv,
                                               fav_stream_encode_png_colors against fav_stream_encode_png, the two operators
  python scripts/color_ab.py parent <dir>      a built checkout of the parent commit in <dir> (its library and binding): the two plain
                                               encodes only, to show that they did not move
Appends to $FAV_AB_OUT/color_ab.log (default: build/color_ab.log, which git ignores)."""
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
log = open(os.path.join(OUT, "color_ab.log"), "a")


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
px = H * W
dev = torch.device("cuda:0")
ck = os.path.join(OUT, "synthetic_model.t7")
if not os.path.exists(ck):
    t7.make_synthetic_checkpoint(ck, seed=1)
net = fav_amd.Net(ck, 0)
st = fav_amd.Stream(net, H, W)
frame_np = synth.smooth_frame(H, W, 1)
frame = torch.from_numpy(frame_np).to(dev)
st.first_frame(frame)
torch.cuda.synchronize()
say(f"[{MODE}] library {fav_amd.LIB_PATH}; {W}x{H}; per call: median (min .. max) over 7 rounds of 200 back-to-back calls, hipEvents")
FORMATS = (("420 centre, BT.709, limited", fav_amd.yuv_format(0, 0, 1, 0), ("420", "center", "709", False)),
           ("444, BT.709, limited", fav_amd.yuv_format(1, 0, 1, 0), ("444", "center", "709", False)))
png, nb = st.png_buffers()
m_png, lo, hi = timed(lambda: st.encode_png_into(png, nb))
say(f"[{MODE}] fav_stream_encode_png                  {m_png:8.2f} us  ({lo:.2f} .. {hi:.2f})   file {int(nb.item())} bytes")
plain = {}
for name, cf, _ in FORMATS:
    buf = torch.empty(fav_amd.yuv_frame_bytes(W, H, cf), dtype=torch.uint8, device=dev)
    plain[name], lo, hi = timed(lambda: st.encode_yuv_into(buf, cf))
    say(f"[{MODE}] fav_stream_encode_yuv ({name})  {plain[name]:8.2f} us  ({lo:.2f} .. {hi:.2f})")
if MODE == "new":
    import color_model as CM
    import yuv_model as M
    state = st.state()
    state_np = state.cpu().numpy()
    m, lo, hi = timed(lambda: st.encode_png_colors_into(frame, fav_amd.YUV_BT709, png, nb))
    say(f"[new] fav_stream_encode_png_colors (BT.709)     {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   file {int(nb.item())} bytes; {m / m_png:.2f} x the plain encode")
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    m, lo, hi = timed(lambda: fav_amd.color_transfer(state, frame, fav_amd.YUV_BT709, out=rgb))
    byts = 15 * px + 3 * px
    say(f"[new] fav_color_transfer_rgb8 (BT.709)          {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   {byts / 1e6:.2f} MB moved -> {byts / m / 1e6:.2f} TB/s (inputs stay in the Infinity Cache between calls)")
    say(f"[new]   equals the fp32 model at 1280x720: {bool(np.array_equal(rgb.cpu().numpy(), CM.transfer(state_np, frame_np, '709')))}")
    for name, cf, f in FORMATS:
        f = M.Format(*f)
        n = fav_amd.yuv_frame_bytes(W, H, cf)
        buf = torch.empty(n, dtype=torch.uint8, device=dev)
        m, lo, hi = timed(lambda: st.encode_yuv_colors_into(frame, buf, cf))
        byts = 15 * px + n
        say(f"[new] fav_stream_encode_yuv_colors ({name})  {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   {byts / 1e6:.2f} MB moved -> {byts / m / 1e6:.2f} TB/s; {m / plain[name]:.2f} x the plain encode")
        say(f"[new]   equals the fp32 model at 1280x720: {bool(np.array_equal(buf.cpu().numpy(), CM.transfer_yuv(state_np, frame_np, f)))}")
        # cold: 32 distinct states and frames (442 MB, more than the 256 MiB Infinity Cache) in turn
        imgs = [torch.rand(3, H, W, device=dev) for _ in range(32)]
        frs = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev) for _ in range(32)]
        k = [0]
        def cold():
            fav_amd.color_transfer(imgs[k[0] % 32], frs[k[0] % 32], cf, out=buf); k[0] += 1
        m, lo, hi = timed(cold, reps=192)
        say(f"[new] fav_color_transfer_yuv ({name}), 32 inputs in turn (442 MB)  {m:8.2f} us  ({lo:.2f} .. {hi:.2f})   {byts / m / 1e6:.2f} TB/s = {100 * byts / m / 1e6 / 8.0:.0f} % of the 8 TB/s peak")
        def cold_plain():
            fav_amd.rgb_to_yuv(imgs[k[0] % 32], cf, out=buf); k[0] += 1
        m2, lo, hi = timed(cold_plain, reps=192)
        say(f"[new] fav_rgb_f32_to_yuv ({name}), the same 32 states in turn      {m2:8.2f} us  ({lo:.2f} .. {hi:.2f})   the coloured encode is {m / m2:.2f} x")
        del imgs, frs
st.close(); net.close()
