"""Transposed convolutions by output phase (csrc/tconv_pack.h; kernels_tconv.hip): the phase / tap tables, the packed weight order and its
index function, without a GPU.  A scalar double-precision loop in a g++-compiled stub evaluates nn.SpatialFullConvolution with NOTHING but
the header's tables (tconv_ntap / tconv_tap_off / tconv_slot), its index function (tconv_pack_index) and the packed buffer -- the three
things the kernel relies on -- and is compared with torch.nn.functional.conv_transpose2d in fp64."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-artistic-videos_amd", "csrc")

GEOMETRIES = [(3, 2, 1, 1), (5, 2, 2, 1), (3, 3, 1, 2), (1, 2, 0, 1), (9, 2, 4, 1), (5, 4, 2, 3), (4, 2, 1, 0)]      # (k, s, p, adj)
H, W = 5, 7


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    d = tmp_path_factory.mktemp("tconvpack")
    src = d / "tconv.cpp"
    src.write_text('''#include "tconv_pack.h"
#include <cstring>
using namespace fav;
extern "C" long pack(const float* w, int cin, int cout, int cinp, int coutp, int k, int s, int p, float* out)
{
    std::vector<float> v; conv_tconv_pack(w, cin, cout, cinp, coutp, k, s, p, v);
    if (out) memcpy(out, v.data(), v.size() * 4);
    return (long)v.size();
}
extern "C" long packed_floats(int cinp, int coutp, int k) { return (long)tconv_packed_floats(cinp, coutp, k); }
extern "C" void halo(int k, int s, int p, int* lo, int* hi) { *lo = tconv_lo(k, s, p); *hi = tconv_hi(k, s, p); }
// x: [cinp][H][W] floats, pk: the packed weights, out: [coutp][OH][OW] doubles (no bias).  Tables + index function + packed buffer only
extern "C" void eval(const float* x, const float* pk, int cinp, int coutp, int H, int W, int k, int s, int p, int OH, int OW, double* out, int* lo_seen, int* hi_seen)
{
    for (int co = 0; co < coutp; ++co)
        for (int oy = 0; oy < OH; ++oy)
            for (int ox = 0; ox < OW; ++ox) {
                const int cy = oy % s, uy = oy / s, cx = ox % s, ux = ox / s;
                double acc = 0.0;
                for (int jy = 0; jy < tconv_ntap(k, s, p, cy); ++jy)
                    for (int jx = 0; jx < tconv_ntap(k, s, p, cx); ++jx) {
                        const int dy = tconv_tap_off(s, p, cy, jy), dx = tconv_tap_off(s, p, cx, jx);
                        if (dy < *lo_seen) *lo_seen = dy; if (dx < *lo_seen) *lo_seen = dx;
                        if (dy > *hi_seen) *hi_seen = dy; if (dx > *hi_seen) *hi_seen = dx;
                        const int iy = uy + dy, ix = ux + dx;
                        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                        const int slot = tconv_slot(k, s, p, cy, cx, jy, jx);
                        for (int ci = 0; ci < cinp; ++ci)
                            acc += (double)x[((size_t)ci * H + iy) * W + ix] * (double)pk[tconv_pack_index(cinp, k, co, ci, slot)];
                    }
                out[((size_t)co * OH + oy) * OW + ox] = acc;
            }
}
''')
    so = d / "libtconvpack.so"
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.pack.restype = ctypes.c_long; lib.packed_floats.restype = ctypes.c_long
    return lib


def _pack(lib, w, cinp, coutp, k, s, p):
    w = np.ascontiguousarray(w, np.float32)
    cin, cout = w.shape[:2]
    n = lib.pack(ctypes.c_void_p(w.ctypes.data), cin, cout, cinp, coutp, k, s, p, ctypes.c_void_p(0))
    assert n == lib.packed_floats(cinp, coutp, k) == coutp // 32 * (cinp // 8) * k * k * 256
    out = np.full(n, np.nan, np.float32)
    lib.pack(ctypes.c_void_p(w.ctypes.data), cin, cout, cinp, coutp, k, s, p, ctypes.c_void_p(out.ctypes.data))
    return out


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(11)
    return {cin: rng.standard_normal((cin, H, W)).astype(np.float32) for cin in (8, 24)}


@pytest.mark.parametrize("k,s,p,adj", GEOMETRIES)
def test_tables_index_and_pack_evaluate_the_transposed_convolution(stub, inputs, k, s, p, adj):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(100 * k + 10 * s + p)
    lo, hi = ctypes.c_int(), ctypes.c_int()
    stub.halo(k, s, p, ctypes.byref(lo), ctypes.byref(hi))
    for cin in (8, 24):
        x = inputs[cin]
        for cout in (4, 32, 96):
            w = rng.standard_normal((cin, cout, k, k)).astype(np.float32)
            coutp = (cout + 31) // 32 * 32
            pk = _pack(stub, w, cin, coutp, k, s, p)
            # every weight occurs exactly once in the pack, and the rest is zero
            assert np.array_equal(np.sort(pk[pk != 0]), np.sort(w.ravel())) and np.count_nonzero(pk) == w.size
            OH, OW = (H - 1) * s - 2 * p + k + adj, (W - 1) * s - 2 * p + k + adj
            got = np.empty((coutp, OH, OW), np.float64)
            lo_seen, hi_seen = ctypes.c_int(0), ctypes.c_int(0)
            stub.eval(ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(pk.ctypes.data), cin, coutp, H, W, k, s, p, OH, OW,
                      ctypes.c_void_p(got.ctypes.data), ctypes.byref(lo_seen), ctypes.byref(hi_seen))
            ref = F.conv_transpose2d(torch.from_numpy(x)[None].double(), torch.from_numpy(w).double(), None, stride=s, padding=p, output_padding=adj)[0].numpy()
            assert ref.shape == (cout, OH, OW)
            err = np.abs(got[:cout] - ref).max()
            assert err <= 1e-5 * np.abs(ref).max(), (cin, cout, err)
            assert not got[cout:].any()                                   # padded output channels: zero filters
            assert (lo_seen.value, hi_seen.value) == (lo.value, hi.value) and lo.value <= 0 <= hi.value      # the halo the kernel stages


@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (5, 4, 2), (4, 2, 1)])
def test_group_blocks_are_the_packings_of_their_filters(stub, k, s, p):
    """wider layers: block g (one tile of 32 output channels, what one wave streams) = the pack of filters 32 g .. 32 g + 31 alone"""
    rng = np.random.default_rng(k)
    for cin, cinp, cout in ((24, 24, 96), (7, 8, 64), (16, 16, 40)):
        w = rng.standard_normal((cin, cout, k, k)).astype(np.float32)
        coutp = (cout + 31) // 32 * 32
        whole = _pack(stub, w, cinp, coutp, k, s, p)
        blk = whole.size // (coutp // 32)
        for g in range(coutp // 32):
            assert np.array_equal(whole[g * blk:(g + 1) * blk], _pack(stub, w[:, 32 * g:32 * g + 32], cinp, 32, k, s, p))
