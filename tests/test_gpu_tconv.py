"""Transposed convolutions by output phase (kernels_tconv.hip, CK_TCONV): the operator against fp64 conv_transpose2d for every geometry
class of the `f<k>s<s>-<n>` grammar, networks with `u`, `f` and `C` items against the CPU oracle, the zero-stuffed form behind
FAV_NO_TCONV (diagnostic build) as an independent cross-check, and what stays refused."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fav_amd import t7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "fast-artistic-videos_amd", "libfav_diag.so")

pytestmark = pytest.mark.gpu

GEOMETRIES = [(3, 2, 1, 1), (5, 2, 2, 1), (3, 3, 1, 2), (1, 2, 0, 1), (9, 2, 4, 1), (5, 4, 2, 3), (4, 2, 1, 0)]      # (k, s, p, adj)
TILE_H, TILE_W = 8, 32                    # the kernel's tile of input pixels (tconv_pack.h: TCONV_TILE_H / TCONV_TILE_W)
SIZES = [(1, 1), (13, 19), (TILE_H + 1, TILE_W + 1)]
CHANNELS = [(ci, co) for ci in (3, 8, 40) for co in (4, 36, 96)]


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def psnr8(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


# output sizes that are NO multiple of the stride (adj < s - 1): the last output row / column exists in some phases only, so a tile's
# (item, phase) partial can hold a ragged last row or no valid pixel at all (count 0) -- e.g. k=3 s=2 p=1 adj=0 at 9x33: 17x65 outputs
RAGGED = [(3, 2, 1, 0), (5, 4, 2, 0), (3, 3, 1, 1), (2, 4, 0, 0)]


@pytest.mark.parametrize("k,s,p,adj", GEOMETRIES + RAGGED)
def test_operator_matches_fp64_conv_transpose2d(favlib, cuda, poison, k, s, p, adj):
    """raw output and InstanceNorm + ReLU (the per-(tile, phase) statistics and counts of ragged last tiles) within 2e-4 * scale.  The
    binding takes contiguous NCHW tensors only, so nothing can be poisoned around the caller's tensors; the operator's own padded
    buffers (input channels up to a multiple of 8, filters up to 32) and the LDS are: NaN in every CU's LDS and in freed device memory"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(1000 * k + 100 * s + 10 * p + adj)
    worst = 0.0
    poison()
    for (h, w) in SIZES:
        for (cin, cout) in CHANNELS:
            x = rng.standard_normal((cin, h, w)).astype(np.float32)
            wt = (rng.standard_normal((cin, cout, k, k)) * np.sqrt(2.0 * s * s / (cin * k * k))).astype(np.float32)
            b = rng.uniform(-0.5, 0.5, cout).astype(np.float32)
            ref = F.conv_transpose2d(torch.from_numpy(x)[None].double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(),
                                     stride=s, padding=p, output_padding=adj)
            got = favlib.conv_transpose2d(T(x, cuda), T(wt, cuda), T(b, cuda), s, p, adj).cpu().numpy()
            r = ref[0].numpy()
            assert got.shape == r.shape == (cout, (h - 1) * s - 2 * p + k + adj, (w - 1) * s - 2 * p + k + adj)
            err = np.abs(got - r).max() / max(1.0, np.abs(r).max()); worst = max(worst, err)
            assert err <= 2e-4, (h, w, cin, cout, err)
            if r.shape[1] * r.shape[2] < 2:
                continue                      # (a single pixel has no variance to normalise by)
            g = rng.uniform(0.1, 1, cout).astype(np.float32); bt = rng.standard_normal(cout).astype(np.float32)
            rn = F.relu(F.instance_norm(ref, weight=torch.from_numpy(g).double(), bias=torch.from_numpy(bt).double(), eps=1e-5))[0].numpy()
            gn = favlib.conv_transpose2d(T(x, cuda), T(wt, cuda), T(b, cuda), s, p, adj, T(g, cuda), T(bt, cuda), 1e-5, True).cpu().numpy()
            err = np.abs(gn - rn).max() / max(1.0, np.abs(rn).max()); worst = max(worst, err)
            assert err <= 2e-4, ("norm", h, w, cin, cout, err)
    print("tconv operator k=%d s=%d p=%d adj=%d: worst relative error %.3e" % (k, s, p, adj, worst))


def test_stride_one_operator_is_the_ordinary_convolution(favlib, cuda):
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(4)
    x = rng.standard_normal((8, 13, 19)).astype(np.float32)
    wt = (rng.standard_normal((8, 36, 3, 3)) * 0.2).astype(np.float32); b = rng.uniform(-0.5, 0.5, 36).astype(np.float32)
    for p in (0, 1, 2):
        ref = F.conv_transpose2d(torch.from_numpy(x)[None].double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), stride=1, padding=p)[0].numpy()
        got = favlib.conv_transpose2d(T(x, cuda), T(wt, cuda), T(b, cuda), 1, p, 0).cpu().numpy()
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 2e-4 * max(1.0, np.abs(ref).max())


def _conv_list(layers):
    """(transposed?, stride, cout) of every convolution in execution order"""
    out = []
    for L in layers:
        if L["type"] == "conv": out.append((False, L["stride"], L["w"].shape[0]))
        elif L["type"] == "fullconv": out.append((True, L["stride"], L["w"].shape[1]))
        elif L["type"] == "res": out.extend(_conv_list(L["block"]))
    return out


def _expected_tconv_id(cout):
    p2 = 4
    while p2 < cout: p2 *= 2                # channel counts run as the next power of two
    return 800 + (p2 + 31) // 32 * 32


def _is_tconv_id(kid):
    """800 + N, N a multiple of 32 (the other kernels' ids -- 32 | 64 | 128, 200 + N ... 700 + N -- are never 800 modulo 32 above 800)"""
    return kid >= 832 and (kid - 800) % 32 == 0


NETWORKS = [
    # (arch, input channels, instance norm, padding type, H, W)
    ("c9s1-32,d64,d128,R128,u64,u32,c9s1-3", 3, True, "reflect-start", 72, 56),
    ("c9s1-32,d64,d128,R128,u64,u32,c9s1-3", 3, False, "reflect-start", 72, 56),
    ("c9s1-16,d32,d64,C64,R64,f5s2-32,f3s2-16,c9s1-3", 7, True, "reflect-start", 72, 56),
    ("c9s1-16,d32,f3s1-32,U2,c3s1-16,c9s1-3", 7, True, "reflect-start", 72, 56),
    ("c9s1-16,c3s3-32,C32,f3s3-16,c9s1-3", 3, True, "zero", 72, 57),               # no `d`: c3s3 / f3s3 close on multiples of 3
    ("c9s1-16,d32,C32,u16,c9s1-3", 7, True, "zero", 72, 56),
    ("c9s1-16,d32,C32,u16,c9s1-3", 7, True, "reflect", 72, 56),
]


@pytest.mark.parametrize("arch,cin,inorm,ptype,h,w", NETWORKS)
def test_networks_vs_oracle_and_kernel_ids(favlib, oracle, cuda, poison, tmp_path, arch, cin, inorm, ptype, h, w):
    path = str(tmp_path / "m.t7")
    t7.make_synthetic_checkpoint(path, arch=arch, seed=7, in_channels=cin, use_instance_norm=inorm, padding_type=ptype)
    layers = t7.extract_layers(t7.load(path)["model"])
    net = favlib.Net(path, 0)
    assert net.describe() == favlib.describe_layers(layers)
    assert net.output_size(h, w) == (h, w)
    x = (np.random.default_rng(3).standard_normal((cin, h, w)) * 50).astype(np.float32)
    ref = oracle.net_forward(layers, x)
    poison()                                  # NaN in every CU's LDS and in freed device memory: nothing outside the logical tensors may count
    net.profile_enable(True)
    got = net.forward(T(x, cuda)).cpu().numpy()
    assert got.shape == ref.shape == (3, h, w)
    err = np.abs(got - ref).max()
    db = psnr8(oracle.to_u8_hwc(oracle.deprocess(got)), oracle.to_u8_hwc(oracle.deprocess(ref)))
    print("%s [%s, %s]: max-abs %.3e (150*tanh units), %.1f dB" % (arch, "IN" if inorm else "BN", ptype, err, db))
    assert err <= 5e-2 and db >= 50.0, (err, db)
    assert np.abs(ref).std() > 5              # not saturated / not trivial
    ids = [kid for (ms, n, macs, kid) in net.profile_read()]
    convs = _conv_list(layers)
    assert len(ids) == len(convs) and any(tr for tr, _, _ in convs)
    for kid, (tr, s, cout) in zip(ids, convs):
        if tr and s >= 2: assert kid == _expected_tconv_id(cout), (kid, cout, ids)
        else: assert not _is_tconv_id(kid), (kid, ids)    # an ordinary kernel (the stride-1 transposed layer included)


def test_zero_stuffed_form_behind_the_diag_switch_agrees(favlib, oracle, cuda, tmp_path):
    """FAV_NO_TCONV (diagnostic build only, read once per process: a child runs it) puts the `u` layers back on the generic kernel over the
    zero-stuffed input -- another kernel, another summation order, the same network within the network gate"""
    arch, h, w = NETWORKS[0][0], 72, 56
    path = str(tmp_path / "m.t7")
    t7.make_synthetic_checkpoint(path, arch=arch, seed=7, in_channels=3)
    x = (np.random.default_rng(3).standard_normal((3, h, w)) * 50).astype(np.float32)
    np.save(tmp_path / "x.npy", x)
    child = ("import sys, numpy as np, torch; sys.path.insert(0, %r); import fav_amd\n"
             "x = np.load(%r); net = fav_amd.Net(%r, 0); net.profile_enable(True)\n"
             "y = net.forward(torch.from_numpy(x).cuda()).cpu().numpy()\n"
             "np.savez(%r, y=y, ids=np.array([r[3] for r in net.profile_read()]))\n"
             % (os.path.join(ROOT, "fast-artistic-videos_amd", "python"), str(tmp_path / "x.npy"), path, str(tmp_path / "stuffed.npz")))
    subprocess.check_call([sys.executable, "-c", child], env=dict(os.environ, FAV_AMD_LIB=DIAG_LIB, FAV_NO_TCONV="1"), timeout=300)
    z = np.load(tmp_path / "stuffed.npz")
    assert not any(_is_tconv_id(int(i)) for i in z["ids"]), z["ids"]
    got = favlib.Net(path, 0).forward(T(x, cuda)).cpu().numpy()
    err = np.abs(got - z["y"]).max()
    db = psnr8(oracle.to_u8_hwc(oracle.deprocess(got)), oracle.to_u8_hwc(oracle.deprocess(z["y"])))
    assert err <= 5e-2 and db >= 50.0, (err, db)


def test_four_channel_producer_in_front_of_a_transposed_layer(favlib, oracle, cuda, tmp_path):
    """a 4-filter producer gives its consumer a channel pitch of 4, which the phase kernel (groups of 8 input channels) does not take: `u<n>`
    (stride 2, adj 1) then runs zero-stuffed on the generic kernel as it always did; any other geometry is refused at load, never run as
    if it were stride 2"""
    path = str(tmp_path / "m.t7")
    t7.make_synthetic_checkpoint(path, arch="c9s1-4,d4,u8,c9s1-3", seed=2, in_channels=3)
    layers = t7.extract_layers(t7.load(path)["model"])
    net = favlib.Net(path, 0)
    assert net.output_size(24, 32) == (24, 32)
    x = (np.random.default_rng(3).standard_normal((3, 24, 32)) * 50).astype(np.float32)
    net.profile_enable(True)
    got = net.forward(T(x, cuda)).cpu().numpy()
    ref = oracle.net_forward(layers, x)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 5e-2
    assert not any(_is_tconv_id(kid) for (ms, n, macs, kid) in net.profile_read())
    for arch in ("c9s1-4,f3s3-8,c9s1-3", "c9s1-4,f5s4-8,c9s1-3"):
        t7.make_synthetic_checkpoint(path, arch=arch, seed=2, in_channels=3)
        with pytest.raises(favlib.FavError, match="behind 4 input channels is unsupported") as e:
            favlib.Net(path, 0)
        assert "libfav error -4:" in str(e.value)
    # ... and stride 2 with adj 0 (not in the `f` grammar: written by hand), which the zero-stuffed x2 map would get wrong
    model = t7.build_model("c9s1-4,u8,c9s1-3", seed=2, in_channels=3)
    full = next(m for m in model["modules"] if m.cls == "nn.SpatialFullConvolution")
    full.fields["adjW"] = full.fields["adjH"] = 0
    t7.write_checkpoint(path, {"model": model})
    with pytest.raises(favlib.FavError, match="behind 4 input channels is unsupported"):
        favlib.Net(path, 0)


def test_what_stays_refused(favlib, cuda, tmp_path):
    x = np.zeros((7, 24, 32), np.float32)
    for arch, text in (("c9s1-16,d32,U2,f3s2-16,c9s1-3", "directly after an upsampling"), ("c9s1-16,d32,f3s2-3", "as the last layer")):
        path = str(tmp_path / "r.t7")
        t7.make_synthetic_checkpoint(path, arch=arch, seed=1)
        net = favlib.Net(path, 0)
        with pytest.raises(favlib.FavError, match=text) as e:
            net.forward(T(x, cuda))
        assert "libfav error -4:" in str(e.value)                      # FAV_EUNSUPPORTED
    with pytest.raises(ValueError, match="odd filter size"):
        t7.build_model("c9s1-16,d32,f4s2-16,c9s1-3")
