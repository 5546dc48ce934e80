"""Lifetime of the C-ABI objects that own device memory, events and queues (fav_net, fav_stream, fav_vr): creating, using and destroying
one over and over must not lower the device's free memory.

Method (every case): the free memory torch.cuda.mem_get_info() reports, after a synchronise.  One create / use / destroy cycle first (the
runtime and torch's allocator keep the pools they grow there); the object's footprint = the drop in free memory while one object is
live in the second cycle; then, over 8 further cycles, free memory after the last must not be lower than after the first by more than
HALF of one footprint.  A leak of one object per cycle exceeds that 16-fold.  Every tensor a cycle passes in is made once, outside it.

The rejected create: fav_vr_create's cube-map crop check behind its allocations ("overlap/2 must be >= 3*floor(median/2)") cannot fail
through the C ABI -- the argument checks in front of it admit only even overlaps >= 12 and median filters <= 5, and 12 / 2 >= 3 * (5 // 2)
-- and no other rejection follows an allocation except a failing HIP call, which a test must not force.  The case therefore uses the
rejection that is reachable (overlap 10: FAV_EINVAL from the argument check) and holds it to the same memory condition."""
import ctypes as C

import numpy as np
import pytest

from fav_amd import synth, t7

pytestmark = pytest.mark.gpu

H, W = 32, 48
ARCH = "c9s1-8,d16,R16,U2,c9s1-3"      # the smallest video architecture the GPU tests build (test_gpu_parity.py)
CYCLES = 8


def _free(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _hold_steady(torch, cycle, name):
    """cycle(probe): one create / use / destroy; calls probe() once while its object is live"""
    cycle(lambda: None)                                     # warm-up
    live = []
    before = _free(torch)
    cycle(lambda: live.append(_free(torch)))
    footprint = before - live[0]
    first = _free(torch)
    for _ in range(CYCLES - 1):
        cycle(lambda: None)
    last = _free(torch)
    print(f"{name}: footprint {footprint} B, free after cycle 1 {first} B, after cycle {CYCLES} {last} B (lost {first - last} B)")
    assert footprint >= 0, (name, footprint)
    assert first - last <= footprint // 2, (name, footprint, first, last)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("lifetime") / "small.t7")
    t7.make_synthetic_checkpoint(p, arch=ARCH, seed=3)
    return p


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_net_load_destroy(favlib, cuda, ckpt):
    import torch

    def cycle(probe):
        net = favlib.Net(ckpt, 0)
        probe()
        net.close()
    _hold_steady(torch, cycle, "fav_net")


def test_stream_every_lazy_resource(favlib, cuda, ckpt):
    """first frame, a next frame with the 4-argument check inline, one look-ahead mask, one asynchronous PNG encode (encoder queue, events,
    second state buffer, workspace), the scaled single-image buffers on and off"""
    import torch
    net = favlib.Net(ckpt, 0)
    f0, f1, f2 = (_dev(synth.smooth_frame(H, W, s), cuda) for s in (1, 2, 3))
    bw = synth.backward_flow(H, W, 4); fw = synth.forward_flow_from_backward(bw, 5)
    bw, fw = _dev(bw, cuda), _dev(fw, cuda)

    def cycle(probe):
        st = favlib.Stream(net, H, W)
        st.first_frame(f0)
        st.next_frame_flow(f1, bw, fw, use_structure=True)
        st.prefetch_mask(f2, bw, fw, use_structure=True)
        out, nbytes = st.png_buffers()
        st.encode_png_async_into(out, nbytes)
        st.wait_png()
        st.set_single_image_size(H - 8, W - 8)
        st.set_single_image_size(0, 0)
        probe()
        torch.cuda.synchronize()
        st.close()
        del out, nbytes
    _hold_steady(torch, cycle, "fav_stream")
    net.check()
    net.close()


def test_vr_with_lookahead(favlib, cuda, ckpt):
    """32 x 32 faces, overlap 12: the first frame's six faces, then face 7 through a look-ahead mask (side queue, its event, the slot,
    the side queue's structure workspace) and face 8 checked inline (the caller's queue's workspace)"""
    import torch
    hp = 32
    net = favlib.Net(ckpt, 0)
    faces = [_dev(synth.smooth_frame(hp, hp, 10 + k), cuda) for k in range(8)]
    bw = synth.backward_flow(hp, hp, 30); fw = synth.forward_flow_from_backward(bw, 31)
    bw, fw = _dev(bw, cuda), _dev(fw, cuda)

    def cycle(probe):
        vr = favlib.VR(net, hp, hp, overlap_w=12, overlap_h=12)
        for k in range(6):
            vr.face_flow(k + 1, faces[k])
        vr.finish_frame()
        vr.prefetch_mask(7, faces[6], bw, fw, use_structure=True)
        vr.face_flow(7, faces[6], bw, fw, use_structure=True)
        vr.face_flow(8, faces[7], bw, fw, use_structure=True)
        probe()
        torch.cuda.synchronize()
        vr.close()
    _hold_steady(torch, cycle, "fav_vr")
    net.check()
    net.close()


def test_vr_rejected_create(favlib, cuda, ckpt):
    import torch
    net = favlib.Net(ckpt, 0)
    L = favlib.lib()
    L.fav_vr_create.restype = C.c_int
    live = favlib.VR(net, 32, 32, overlap_w=12, overlap_h=12)      # the footprint of the object a rejected create must not leave behind
    with_one = _free(torch)
    live.close()
    footprint = _free(torch) - with_one
    opts = favlib._VROpts(10, 10, 7, 3, 0, 1, 0, 0, 0, 0, favlib.BORDER_STN)
    free = []
    for _ in range(1 + CYCLES):                                        # (the first one warms up)
        h = C.c_void_p()
        assert L.fav_vr_create(net.h, None, 32, 32, C.byref(opts), C.byref(h)) == -1      # FAV_EINVAL
        assert not h.value
        free.append(_free(torch))
    print(f"rejected fav_vr_create: footprint of an accepted one {footprint} B, free after rejection 1 {free[1]} B, after rejection {CYCLES} {free[-1]} B")
    assert footprint >= 0 and free[1] - free[-1] <= footprint // 2, (footprint, free)
    net.close()
