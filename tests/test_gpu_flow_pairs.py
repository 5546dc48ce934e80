"""The batched bidirectional flow estimator on the GPU (fav_flow_pairs_rgb8: csrc/kernels_flow.hip with blockIdx.z as the item,
csrc/flow.cpp), what the six cube faces of a 360-degree frame need.

No tolerance anywhere: every output of the batch must be bit-identical to what the single-pair entry fav_flow_rgb8 writes for the same
(A, B, options) -- and that entry is held to the numpy model and to bin/fav_flow by tests/test_gpu_flow.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402
from flow_testing import dev as _dev  # noqa: E402

pytestmark = pytest.mark.gpu


_pairs = {}


def _pair(h, w, slot, cuda):
    """(prev, cur) of a slot on the device: flow_model.warped_pair with a seed of the slot's own"""
    if (h, w, slot) not in _pairs:
        A, B = M.warped_pair(h, w, 100 + 7 * slot)
        _pairs[(h, w, slot)] = (_dev(A, cuda), _dev(B, cuda))
    return _pairs[(h, w, slot)]


_singles = {}


def _single(favlib, h, w, slot, cuda, **opts):
    """(backward, forward) of a slot from fav_flow_rgb8, computed once per (size, slot, options) and never written"""
    key = (h, w, slot, tuple(sorted(opts.items())))
    if key not in _singles:
        prev, cur = _pair(h, w, slot, cuda)
        _singles[key] = (favlib.flow_rgb8(cur, prev, **opts), favlib.flow_rgb8(prev, cur, **opts))
    return _singles[key]


def _assert_equal(got, want, what):
    import torch
    assert got.shape == want.shape and torch.equal(got, want), what


# ------------------------------------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize("h,w,n", [(17, 23, 6), (64, 64, 6), (150, 203, 6), (64, 64, 1), (64, 64, 2), (64, 64, 8)])
def test_pairs_equal_the_single_pair_estimator_bit_for_bit(favlib, cuda, h, w, n):
    slots = [_pair(h, w, k, cuda) for k in range(n)]
    bw, fw = favlib.flow_pairs([p for p, _ in slots], [c for _, c in slots])
    assert len(bw) == n and len(fw) == n
    for k in range(n):
        wb, wf = _single(favlib, h, w, k, cuda)
        _assert_equal(bw[k], wb, f"backward flow of slot {k}")
        _assert_equal(fw[k], wf, f"forward flow of slot {k}")
    if n > 1:                                               # distinct content per slot: the comparison tells the slots apart
        import torch
        assert not torch.equal(bw[0], bw[1])


# ------------------------------------------------------------------------------------------------ 2. items do not leak
def test_items_do_not_leak_into_each_other(favlib, cuda):
    import torch
    h, w = 64, 64
    (p0, c0), (p2, c2) = _pair(h, w, 0, cuda), _pair(h, w, 2, cuda)
    same = _pair(h, w, 1, cuda)[0]
    bw, fw = favlib.flow_pairs([p0, same, p2], [c0, same, c2])
    assert not bw[1].any() and not fw[1].any()             # identical images: exactly zero, both directions
    assert bw[0].any() and fw[2].any()
    rb, rf = favlib.flow_pairs([p2, same, p0], [c2, same, c0])
    for k in range(3):
        assert torch.equal(rb[2 - k], bw[k]) and torch.equal(rf[2 - k], fw[k]), k
    for k in (0, 2):
        wb, wf = _single(favlib, h, w, k, cuda)
        assert torch.equal(bw[k], wb) and torch.equal(fw[k], wf), k


# ------------------------------------------------------------------------------------------------ 3. blocking independence
def test_batch_does_not_depend_on_sweeps_per_launch(favlib, cuda):
    """iters 15: 15 launches of 1, 2 of 6 + a remainder of 3, one of 15 under a bound of 16"""
    import torch
    h, w = 150, 203
    slots = [_pair(h, w, k, cuda) for k in range(2)]
    prev, cur = [p for p, _ in slots], [c for _, c in slots]
    base = favlib.flow_pairs(prev, cur, dict(iters=15, sweeps_per_launch=1))
    for spl in (6, 16):
        got = favlib.flow_pairs(prev, cur, dict(iters=15, sweeps_per_launch=spl))
        for k in range(2):
            assert torch.equal(got[0][k], base[0][k]) and torch.equal(got[1][k], base[1][k]), (spl, k)
    for k in range(2):
        wb, wf = _single(favlib, h, w, k, cuda, iters=15)
        assert torch.equal(base[0][k], wb) and torch.equal(base[1][k], wf), k


# ------------------------------------------------------------------------------------------------ 4. poison
def test_pairs_after_poison(favlib, cuda, poison):
    import torch
    h, w, n = 150, 203, 2
    slots = [_pair(h, w, k, cuda) for k in range(n)]
    prev, cur = [p for p, _ in slots], [c for _, c in slots]
    want = [_single(favlib, h, w, k, cuda) for k in range(n)]
    nb = favlib.flow_pairs_workspace_bytes(w, h, n)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    poison()
    for fill in ("nan", "0x7f"):
        if fill == "nan":
            ws = torch.full(((nb + 3) // 4,), float("nan"), dtype=torch.float32, device=cuda)
            outs = [torch.full((h, w, 2), float("nan"), dtype=torch.float32, device=cuda) for _ in range(2 * n)]
        else:
            ws = torch.full((nb,), 0x7f, dtype=torch.uint8, device=cuda)
            outs = [torch.full((h, w, 8), 0x7f, dtype=torch.uint8, device=cuda).view(torch.float32) for _ in range(2 * n)]
        favlib._check(favlib.lib().fav_flow_pairs_rgb8(arr(prev), arr(cur), n, w, h, None, arr(outs[:n]), arr(outs[n:]), favlib._p(ws), C.c_size_t(nb),
                                                       favlib._stream()))
        for k in range(n):
            assert torch.isfinite(outs[k]).all() and torch.equal(outs[k], want[k][0]), (fill, k)
            assert torch.isfinite(outs[n + k]).all() and torch.equal(outs[n + k], want[k][1]), (fill, k)


# ------------------------------------------------------------------------------------------------ 5. one shared image
def test_one_image_in_two_slots(favlib, cuda):
    """a three-frame chain f0 -> f1 -> f2 as two pairs: prev[0] is cur[1]"""
    import torch
    (f0, f1), f2 = _pair(64, 64, 0, cuda), _pair(64, 64, 1, cuda)[1]
    bw, fw = favlib.flow_pairs([f1, f0], [f2, f1])
    assert torch.equal(bw[0], favlib.flow_rgb8(f2, f1)) and torch.equal(fw[0], favlib.flow_rgb8(f1, f2))
    assert torch.equal(bw[1], favlib.flow_rgb8(f1, f0)) and torch.equal(fw[1], favlib.flow_rgb8(f0, f1))


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors_enqueue_nothing(favlib, cuda):
    import torch
    h, w, n = 64, 64, 2
    slots = [_pair(h, w, k, cuda) for k in range(n)]
    prev, cur = [p for p, _ in slots], [c for _, c in slots]
    nb = favlib.flow_pairs_workspace_bytes(w, h, n)
    ws = torch.full((nb + 16,), 0x55, dtype=torch.uint8, device=cuda)
    outs = [torch.full((h, w, 2), -7.0, dtype=torch.float32, device=cuda) for _ in range(2 * n)]
    L = favlib.lib()
    ptrs = lambda ts: [t.data_ptr() if t is not None else None for t in ts]
    ok = dict(prev=ptrs(prev), cur=ptrs(cur), bw=ptrs(outs[:n]), fw=ptrs(outs[n:]), ws=ws.data_ptr(), nb=nb, n=n)
    assert ws.data_ptr() % 16 == 0

    def call(**kw):
        a = dict(ok, **kw)
        arr = lambda v: (C.c_void_p * len(v))(*v)
        return L.fav_flow_pairs_rgb8(arr(a["prev"]), arr(a["cur"]), a["n"], w, h, None, arr(a["bw"]), arr(a["fw"]), C.c_void_p(a["ws"]),
                                     C.c_size_t(a["nb"]), favlib._stream())

    nine = lambda v: (v * 5)[:9]
    cases = ((dict(n=0), "n_pairs must be 1 .. 8, not 0"),
             (dict(n=9, prev=nine(ok["prev"]), cur=nine(ok["cur"]), bw=nine(ok["bw"]), fw=nine(ok["fw"])), "n_pairs must be 1 .. 8, not 9"),
             (dict(prev=[ok["prev"][0], None]), "null pointer in slot 1"), (dict(fw=[None, ok["fw"][1]]), "null pointer in slot 0"),
             (dict(fw=[ok["fw"][0], ok["bw"][0]]), "two outputs are one buffer (backward_flo[0] and forward_flo[1])"),
             (dict(nb=nb - 1), f"the workspace holds {nb - 1} bytes"),
             (dict(ws=ws.data_ptr() + 8), "the workspace must be 16-byte aligned"))
    for kw, msg in cases:
        assert call(**kw) == -1, kw                                                         # FAV_EINVAL
        assert msg.encode() in L.fav_last_error(), (kw, L.fav_last_error())
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs) and bool((ws == 0x55).all())         # nothing ran
    assert call() == 0                                                                      # the same arguments, unbroken: it runs
    assert torch.equal(outs[0], _single(favlib, h, w, 0, cuda)[0]) and torch.equal(outs[n + 1], _single(favlib, h, w, 1, cuda)[1])


# ------------------------------------------------------------------------------------------------ 7. the stream: the batch of one
def test_stream_estimate_with_the_pairs_workspace_equals_the_single_calls(favlib, cuda):
    """fav_stream_next_frame_estimate with fav_flow_pairs_workspace_bytes(W, H, 1) (what bin/fav_stylize -estimate_flow 1 passes) runs both
    flows as the batch of one; with fav_flow_workspace_bytes it makes two single calls: flows, mask, state and PNGs are the same bits"""
    import torch
    h, w = 64, 96
    net = favlib.Net(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_model.t7"), 0)
    A, B = M.warped_pair(h, w, 31)
    frames = [_dev(f, cuda) for f in (A, B, A)]              # there and back: both flows exist at either step
    assert favlib.flow_pairs_workspace_bytes(w, h, 1) > favlib.flow_workspace_bytes(w, h)
    results = []
    for batched in (False, True):
        st = favlib.Stream(net, h, w)
        st.first_frame(frames[0])
        pngs = [favlib.png_encode(None, from_stream=st)]
        for i in (1, 2):
            _, _, bw, fw = st.next_frame_estimate(frames[i], frames[i - 1], use_structure=True, batched=batched)
            assert torch.equal(bw, favlib.flow_rgb8(frames[i], frames[i - 1])) and torch.equal(fw, favlib.flow_rgb8(frames[i - 1], frames[i])), i
            pngs.append(favlib.png_encode(None, from_stream=st))
        results.append((st.state().cpu().numpy(), pngs, st.last_mask().cpu().numpy()))
        st.close()
    (s0, p0, m0), (s1, p1, m1) = results
    assert np.array_equal(s0, s1) and p0 == p1 and np.array_equal(m0, m1) and len(p0) == 3
    assert (m0 == 255).any()                                 # the estimated flows are consistent somewhere: the prior is used
