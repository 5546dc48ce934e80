"""Host side of the batched bidirectional flow estimator (fav_flow_pairs_rgb8; no GPU needed): the workspace size, the exported symbols
and the argument checks that come before any device is touched."""
import ctypes as C
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _r256(n):
    return (n + 255) // 256 * 256


def test_pairs_workspace_bytes(favlib):
    L = favlib.lib()
    for w, h, n, msg in ((64, 64, 0, "n_pairs must be 1 .. 8"), (64, 64, 9, "n_pairs must be 1 .. 8"), (64, 64, -1, "n_pairs must be 1 .. 8"),
                         (15, 64, 2, "at least 16x16"), (64, 15, 2, "at least 16x16")):
        assert L.fav_flow_pairs_workspace_bytes(w, h, n, None) == 0 and msg.encode() in L.fav_last_error(), (w, h, n)
    o = favlib._flow_opts({"levels": 7})
    assert L.fav_flow_pairs_workspace_bytes(64, 64, 2, C.cast(C.pointer(o), C.c_void_p)) == 0 and b"levels must be" in L.fav_last_error()
    with pytest.raises(favlib.FavError, match="n_pairs must be"):
        favlib.flow_pairs_workspace_bytes(64, 64, 9)
    for (h, w) in M.SIZES + [(720, 1280)]:
        sizes = [favlib.flow_pairs_workspace_bytes(w, h, n) for n in range(1, favlib.FLOW_MAX_PAIRS + 1)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
        # one pair: at least what one flow of the single-pair entry needs (two grey pyramids, its flow buffers, its coefficients)
        assert sizes[0] >= favlib.flow_workspace_bytes(w, h)
        # the layout: per image a grey pyramid; per flow two flow buffers a level (level 0: one, the other is the caller's) and one
        # coefficient image of 16 B per pixel; 256-byte sections
        for n, got in zip(range(1, favlib.FLOW_MAX_PAIRS + 1), sizes):
            lv = M.level_sizes(h, w)
            want = sum(2 * n * _r256(lh * lw * 4) + 2 * n * (2 if l else 1) * _r256(lh * lw * 8) for l, (lh, lw) in enumerate(lv)) + 2 * n * _r256(h * w * 16)
            assert got == want, (h, w, n)
    assert favlib.flow_pairs_workspace_bytes(64, 64, 2, levels=1) < favlib.flow_pairs_workspace_bytes(64, 64, 2)


def test_pairs_exports_and_argument_checks_before_the_device(favlib):
    out = subprocess.run(["nm", "-D", "--defined-only", favlib.LIB_PATH], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ("fav_flow_pairs_workspace_bytes", "fav_flow_pairs_rgb8"):
        assert name in defined and name in favlib.EXPORTS, name
    assert callable(favlib.flow_pairs)
    hdr = open(os.path.join(ROOT, "include", "fav.h")).read()
    assert "#define FAV_FLOW_MAX_PAIRS 8" in hdr and favlib.FLOW_MAX_PAIRS == 8
    L = favlib.lib()
    P = lambda *v: (C.c_void_p * len(v))(*v)
    nb = favlib.flow_pairs_workspace_bytes(64, 64, 2)
    ok = dict(prev=P(256, 512), cur=P(768, 1024), bw=P(4096, 8192), fw=P(12288, 16384), ws=C.c_void_p(1 << 20), nb=nb, n=2, w=64, h=64)

    def call(**kw):
        a = dict(ok, **kw)
        return L.fav_flow_pairs_rgb8(a["prev"], a["cur"], a["n"], a["w"], a["h"], None, a["bw"], a["fw"], a["ws"], C.c_size_t(a["nb"]), None)

    for kw, msg in ((dict(n=0), "n_pairs must be 1 .. 8, not 0"), (dict(n=9), "n_pairs must be 1 .. 8, not 9"), (dict(w=15), "at least 16x16"),
                    (dict(prev=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(cur=P(768, None)), "null pointer in slot 1"),
                    (dict(fw=P(12288, 4096)), "two outputs are one buffer (backward_flo[0] and forward_flo[1])"),
                    (dict(bw=P(4096, 4096)), "two outputs are one buffer (backward_flo[0] and backward_flo[1])"),
                    (dict(bw=P(4100, 8192)), "8-byte aligned"), (dict(nb=nb - 1), f"workspace holds {nb - 1} bytes"),
                    (dict(ws=C.c_void_p((1 << 20) + 8)), "workspace must be 16-byte aligned")):
        assert call(**kw) == -1 and msg.encode() in L.fav_last_error(), (kw, L.fav_last_error())
    import torch
    if not torch.cuda.is_available():      # valid arguments, no device: FAV_ENODEVICE before anything is dereferenced
        assert call() == -6 and b"no CPU fallback" in L.fav_last_error()
