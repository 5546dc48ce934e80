"""The structure map of the 4-argument consistency check as the GPU computes it (csrc/kernels_consistency.hip: moments_t_kernel, the two
recursive passes iir_cols_kernel<22,64> / <14,1024>, the tile transpose, the eigenvalue, normalize's order-dependent min / max, the exact
sequential sum, the packed form's dealing of work by XCD), read VALUE BY VALUE through fav_structure_f32 and held to the reference bit
for bit: uint32 views of the maps, the average as four bytes, no tolerance, no value left out.

Every other test sees the map only through the mask: one comparison per pixel, which a wrong value flips only where the squared
forward-backward error happens to lie within the perturbation of the threshold (tests/test_cpu_structure.py shows a wrong line start that
moves no mask byte).

Reference: oracle.structure (fp32 operations in the reference's order), which tests/test_cpu_structure.py pins on the reference's own
compiled code; the recorded maps of that code (tests/golden/structure_ref_cases.npz); the compiled code itself where it is present.
Sizes and images: tests/util/structure_cases.py -- chosen from the kernels: lines of 2, 3, D-1 .. 2D+1 samples for both ring depths on
both axes, line counts around a wave of 256, the sequential sum's hand-over at 65 536 values.

Nothing stale can pass: before EVERY call the workspace and both outputs are filled with 0xFF bytes (NaN patterns)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import structure_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

PACKED_DEFAULT = [(4, 0), (4, 5)]                                          # (pack_cus, q0) at every size
PACKED_CROSS = [(p, q) for p in (1, 2, 3, 4) for q in range(8)]            # ... and at SC.CROSS_SIZES


@pytest.fixture(scope="module")
def want(oracle):
    """(h, w, kind) -> (image, oracle map, oracle average): computed once per case, shared by every test, never written to"""
    cache = {}

    def get(h, w, kind):
        key = (h, w, kind)
        if key not in cache:
            img = SC.image(kind, h, w)
            m, avg = oracle.structure(img)
            assert np.isfinite(m).all() and np.isfinite(avg), key         # (bit equality below would let NaN == NaN patterns through)
            for a in (img, m):
                a.flags.writeable = False
            cache[key] = (img, m, avg)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def expect_packed(cuda):
    """an MI355X presents eight XCDs: there a packed call that ran the wide form would make these tests pass vacuously"""
    import torch
    p = torch.cuda.get_device_properties(cuda)
    return getattr(p, "gcnArchName", "").startswith("gfx950") and p.multi_processor_count == 256


class Runner:
    """one frame size: workspace and outputs allocated once, refilled with garbage before every call"""

    def __init__(self, favlib, cuda, h, w):
        import torch
        self.torch, self.fav, self.h, self.w = torch, favlib, h, w
        self.ws = torch.empty(favlib.lib().fav_consistency_workspace_bytes(w, h, 1), dtype=torch.uint8, device=cuda)
        self.out8 = torch.empty(h * w * 4, dtype=torch.uint8, device=cuda)
        self.avg8 = torch.empty(4, dtype=torch.uint8, device=cuda)

    def fill(self, garbage=None):
        if garbage is None:
            for t in (self.ws, self.out8, self.avg8): t.fill_(0xFF)
        else:                                                             # seeded random bytes
            g = self.torch.Generator(device=self.ws.device); g.manual_seed(garbage)
            for t in (self.ws, self.out8, self.avg8): t.random_(0, 256, generator=g)

    def __call__(self, frame, pack_cus=0, q0=0, garbage=None):
        self.fill(garbage)
        out, avg, form = self.fav.structure(frame, pack_cus, q0, ws=self.ws, out=self.out8.view(self.torch.float32).view(self.h, self.w),
                                            avg=self.avg8.view(self.torch.float32))
        return out.cpu().numpy(), avg.cpu().numpy()[0], form


def _check_forms(run, frame, m, avg, forms, expect_packed, label):
    """wide against the reference; every packed form against the reference AND against the wide result"""
    wm, wavg, form = run(frame)
    assert form == run.fav.STRUCTURE_WIDE
    SC.same_bits(wm, wavg, m, avg, f"{label}, wide form vs oracle")
    for (pack, q0) in forms:
        pm, pavg, form = run(frame, pack, q0)
        if expect_packed:
            assert form == run.fav.STRUCTURE_PACKED, f"{label}: pack_cus {pack} ran the wide form on a device with eight XCDs"
        SC.same_bits(pm, pavg, m, avg, f"{label}, packed form pack_cus={pack} q0={q0} (form_ran {form}) vs oracle")
        SC.same_bits(pm, pavg, wm, wavg, f"{label}, packed form pack_cus={pack} q0={q0} (form_ran {form}) vs wide form")
    return wm, wavg


@pytest.mark.parametrize("size", SC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_structure_map_bit_exact(favlib, cuda, want, expect_packed, size):
    """every size x every image kind: wide, and packed with pack_cus = 4 at q0 = 0 and 5"""
    import torch
    h, w = size
    run = Runner(favlib, cuda, h, w)
    for kind in SC.KINDS:
        img, m, avg = want(h, w, kind)
        _check_forms(run, torch.tensor(img, device=cuda), m, avg, PACKED_DEFAULT, expect_packed, f"{kind} {h}x{w}")


@pytest.mark.parametrize("size", SC.CROSS_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_share_count_and_placement_gives_the_same_bits(favlib, cuda, want, expect_packed, size):
    """pack_cus 1..4 x q0 0..7: stand-alone, the eight blocks of a launch land one per XCD, so every q0 is a valid placement and every
    share count must deal ALL the work -- a share computed by nobody leaves the 0xFF fill behind"""
    import torch
    h, w = size
    run = Runner(favlib, cuda, h, w)
    for kind in SC.KINDS:
        img, m, avg = want(h, w, kind)
        _check_forms(run, torch.tensor(img, device=cuda), m, avg, PACKED_CROSS, expect_packed, f"{kind} {h}x{w}")


def test_structure_map_is_the_recorded_reference_map(favlib, cuda, golden_dir, expect_packed):
    """the recorded results of the reference's compiled code (tests/golden/structure_ref_cases.npz), both forms"""
    import torch
    rec = np.load(os.path.join(golden_dir, "structure_ref_cases.npz"))
    runs = {}
    for (h, w, kind) in SC.FIXTURE_CASES:
        run = runs.setdefault((h, w), Runner(favlib, cuda, h, w))
        _check_forms(run, torch.tensor(rec[f"img_{h}x{w}_{kind}"], device=cuda), rec[f"map_{h}x{w}_{kind}"], rec[f"avg_{h}x{w}_{kind}"],
                     [(4, 3)], expect_packed, f"recorded reference, {kind} {h}x{w}")


def test_structure_map_is_the_live_reference_map(favlib, cuda, oracle, want, expect_packed):
    """the reference's compiled code itself (oracle/_ref/libstructure_ref.so), where it is present: every size, every kind"""
    import torch
    if not oracle.structure_ref_available():
        pytest.skip("oracle/_ref/libstructure_ref.so is not present (built only where the reference tree is)")
    for (h, w) in SC.SIZES:
        run = Runner(favlib, cuda, h, w)
        for kind in SC.KINDS:
            img = want(h, w, kind)[0]
            rm, ravg = oracle.structure_ref(img)
            _check_forms(run, torch.tensor(img, device=cuda), rm, ravg, [(2, 6)], expect_packed, f"live reference, {kind} {h}x{w}")


@pytest.mark.parametrize("size", SC.POISON_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_structure_map_behind_poisoned_lds(favlib, cuda, want, expect_packed, poison, size):
    """one size of each group again with every CU's LDS NaN-filled (the rings of the recursive passes, the scans' tiles live there)"""
    import torch
    h, w = size
    run = Runner(favlib, cuda, h, w)
    for kind in ("smooth", "pixel"):
        img, m, avg = want(h, w, kind)
        frame = torch.tensor(img, device=cuda)
        for (pack, q0) in [(0, 0), (4, 1), (3, 6)]:
            poison()
            gm, gavg, form = run(frame, pack, q0)
            if expect_packed:
                assert form == (favlib.STRUCTURE_PACKED if pack else favlib.STRUCTURE_WIDE)
            SC.same_bits(gm, gavg, m, avg, f"{kind} {h}x{w} behind poisoned LDS, pack_cus={pack} q0={q0}")


@pytest.mark.parametrize("size", [(14, 15), (257, 28), (301, 258)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_structure_map_does_not_depend_on_what_the_buffers_held(favlib, cuda, want, size):
    """two calls over different garbage (0xFF bytes, seeded random bytes) in the workspace and the outputs: the same bits"""
    import torch
    h, w = size
    run = Runner(favlib, cuda, h, w)
    for kind in ("noise", "pixel"):
        img, m, avg = want(h, w, kind)
        frame = torch.tensor(img, device=cuda)
        for (pack, q0) in [(0, 0), (4, 2), (1, 7)]:
            for garbage in (None, 1234 + h, 99 + w):
                gm, gavg, _ = run(frame, pack, q0, garbage)
                SC.same_bits(gm, gavg, m, avg, f"{kind} {h}x{w} over garbage {garbage}, pack_cus={pack} q0={q0}")


def test_structure_map_of_a_frame_at_odd_byte_offsets(favlib, cuda, want, expect_packed):
    """the frame at byte offsets 1 and 3 of its allocation (a u8 image has no alignment to rely on)"""
    import torch
    h, w = 45, 71
    run = Runner(favlib, cuda, h, w)
    img, m, avg = want(h, w, "noise")
    for off in (1, 3):
        buf = torch.full((h * w * 3 + 8,), 0xFF, dtype=torch.uint8, device=cuda)
        buf[off:off + h * w * 3] = torch.tensor(img, device=cuda).reshape(-1)
        frame = buf[off:off + h * w * 3].view(h, w, 3)
        assert frame.data_ptr() % 4 == off and frame.is_contiguous()
        _check_forms(run, frame, m, avg, [(4, 4)], expect_packed, f"noise {h}x{w} at byte offset {off}")


def test_bad_arguments_are_refused_and_nothing_is_written(favlib, cuda, want):
    import torch
    h, w = 14, 15
    run = Runner(favlib, cuda, h, w)
    frame = torch.tensor(want(h, w, "noise")[0], device=cuda)
    L = favlib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(rgb=frame.data_ptr(), W=w, H=h, ws=run.ws.data_ptr(), ws_bytes=run.ws.numel(), out=run.out8.data_ptr(), avg=run.avg8.data_ptr(),
                pack=0, q0=0, form=True)
    bad = [dict(rgb=0), dict(ws=0), dict(out=0), dict(avg=0), dict(form=False), dict(W=1), dict(H=1), dict(W=0), dict(H=-3),
           dict(ws_bytes=run.ws.numel() - 1), dict(ws_bytes=0), dict(pack=-1), dict(pack=5), dict(q0=-1), dict(q0=8), dict(pack=4, q0=8)]
    for change in bad:
        a = dict(good, **change)
        run.fill()
        form = C.c_int(-7)
        rc = L.fav_structure_f32(C.c_void_p(a["rgb"]), a["W"], a["H"], C.c_void_p(a["ws"]), C.c_size_t(a["ws_bytes"]), C.c_void_p(a["out"]),
                                 C.c_void_p(a["avg"]), a["pack"], a["q0"], C.byref(form) if a["form"] else None, stream)
        torch.cuda.synchronize()
        assert rc == -1, (change, rc)                                                                  # FAV_EINVAL
        assert L.fav_last_error().decode().startswith("fav_structure_f32:"), change
        assert form.value == -7, change
        for t in (run.out8, run.avg8, run.ws):
            assert bool((t == 0xFF).all()), f"{change}: a refused call wrote to a buffer"
    with pytest.raises(favlib.FavError):
        favlib.structure(frame, pack_cus=9)
    # ... and the same buffers still serve a good call
    img, m, avg = want(h, w, "noise")
    gm, gavg, _ = run(frame)
    SC.same_bits(gm, gavg, m, avg, "after the refused calls")
