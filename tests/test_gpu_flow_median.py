"""The estimator's median filter (fav_flow_opts_ex3.median) on the GPU against its numpy restatement (tests/util/flow_median_model.py): the
stage entry, the whole estimator through fav_flow_rgb8_ex3, fav_flow_pairs_rgb8_ex3, fav_stream_next_frame_estimate_ex3 and bin/fav_flow
-median, and the _ex3 entries with the option off against the _ex2 entries.

Tolerances: the filter computes nothing, it selects, so the stage must EQUAL the model's sort value for value.  A median is 1-Lipschitz in
the sup norm (|med(x) - med(y)| <= max|x - y|), so the whole estimator with the filter keeps the gates its options already have
(flow_testing.py): with e32 = max|M32 - M64| of the two CPU models on the same input, computed here at every run, max|GPU - M64| <=
max(4 e32, floor) for the plain estimator (gate_floor) and <= 4 e32 with smooth_eps, data_term or match_beta (gate_4e32).  No new
tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import flow_model as M  # noqa: E402
import flow_match_model as P  # noqa: E402
import flow_median_model as D  # noqa: E402
from flow_testing import dev as _dev, gate_floor, gate_4e32, run as _run, write_ppm as _write_ppm  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fast-artistic-videos_amd", "bin")
VID = os.path.join(ROOT, "tests", "golden", "tiny_model.t7")
EPS, SEED = 0.3, 11
MATCH_SCENE = (64, 96, 2, (22, 42, 30, 50), (9.0, -6.0), (1.0, 0.0))          # a 20 x 20 object moving (9, -6) over a background moving (1, 0)


def _inputs(name):
    if name == "match 64x96":
        return P.scene(*MATCH_SCENE)[:2]
    h, w = (int(t) for t in name.split("x"))
    return M.warped_pair(h, w, SEED)


_cases = {}


def _case(name, **opts):
    """(A, B, fp32 model flow, fp64 model flow) of an input with the binding's options, computed once and left unchanged"""
    key = (name, tuple(sorted(opts.items())))
    if key not in _cases:
        A, B = _inputs(name)
        kw = dict(levels=opts.get("levels", 0), warps=opts.get("warps", 0), iters=opts.get("iters", 0), eps=opts.get("smooth_eps", 0.0),
                  grad=bool(opts.get("data_term", 0)), beta=P.BETA if opts.get("match_beta", 0) else 0.0, radius=opts.get("match_radius", 0) or P.RADIUS,
                  median_size=opts.get("median", 0))
        _cases[key] = (A, B, D.flow(A, B, dtype=np.float32, **kw), D.flow(A, B, dtype=np.float64, **kw))
    return _cases[key]


def _flow_into_poisoned_buffers(favlib, cuda, a, b, **opts):
    """fav_flow_rgb8_ex3 with a workspace and an output that hold NaN beforehand"""
    import torch
    h, w = a.shape[0], a.shape[1]
    o = favlib._flow_opts_ex3(opts)
    nb = favlib.flow_workspace_bytes(w, h, **opts)
    ws = torch.full(((nb + 3) // 4,), float("nan"), dtype=torch.float32, device=cuda)
    out = torch.full((h, w, 2), float("nan"), dtype=torch.float32, device=cuda)
    favlib._check(favlib.lib().fav_flow_rgb8_ex3(favlib._p(a), favlib._p(b), w, h, C.byref(o), favlib._p(out), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
    return out


# ------------------------------------------------------------------------------------------------ 1. the stage, exact
STAGE_SHAPES = [(16, 16), (67, 131), (41, 23)]      # (h, w): the smallest frame; ragged in both axes, 3 x 5 tiles; narrower than a tile and taller than two


def test_median_stage_equals_the_model(favlib, cuda, poison):
    """normal noise plus spikes; the output lies between two guard zones that must be intact; LDS holds NaN beforehand"""
    import torch
    GUARD, MARK = 4096, 12345.0
    torch.cuda.synchronize()
    poison()
    for h, w in STAGE_SHAPES:
        rng = np.random.default_rng(h * 1000 + w)
        f = rng.standard_normal((h, w, 2)).astype(np.float32)
        spikes = rng.random((h, w, 2)) < 0.05
        f[spikes] += (rng.choice([-1.0, 1.0], spikes.sum()) * rng.uniform(20, 60, spikes.sum())).astype(np.float32)
        f[0, 0] += np.float32(100.0); f[h - 1, w - 1] -= np.float32(100.0); f[0, w // 2, 0] += np.float32(80.0); f[h // 2, 0, 1] -= np.float32(80.0)
        src = _dev(f, cuda)
        n = h * w * 2
        for size in (3, 5):
            buf = torch.full((GUARD + n + GUARD,), MARK, dtype=torch.float32, device=cuda)
            favlib._check(favlib.lib().fav_flow_median_f32(favlib._p(src), C.c_void_p(buf.data_ptr() + GUARD * 4), w, h, size, favlib._stream()))
            got = buf.cpu().numpy()
            assert (got[:GUARD] == MARK).all() and (got[GUARD + n:] == MARK).all(), (h, w, size)
            want = D.median(f, size)
            out = got[GUARD:GUARD + n].reshape(h, w, 2)
            print(f"median {size}x{size} of {h}x{w}: {int((out != want).sum())} of {n} values differ; {int((want != f).sum())} changed by the filter")
            assert np.array_equal(out, want), (h, w, size)
            assert np.array_equal(favlib.flow_median(src, size).cpu().numpy(), want)          # the binding
            assert np.array_equal(src.cpu().numpy(), f)                                      # the input is not written
    with pytest.raises(favlib.FavError, match="size must be 3 or 5"):
        favlib.flow_median(src, 4)
    with pytest.raises(favlib.FavError, match="overlap"):
        favlib._check(favlib.lib().fav_flow_median_f32(favlib._p(src), favlib._p(src), w, h, 5, favlib._stream()))


# ------------------------------------------------------------------------------------------------ 2. the whole estimator
ESTIMATES = [("64x64", dict(median=5)), ("150x203", dict(median=5)),
             ("64x64", dict(median=3, smooth_eps=EPS)), ("150x203", dict(median=3, smooth_eps=EPS)),
             ("64x64", dict(median=3, data_term=1)), ("150x203", dict(median=3, data_term=1)),
             ("match 64x96", dict(median=3, match_beta=-1))]


@pytest.mark.parametrize("name,opts", ESTIMATES, ids=[f"{n}-{'-'.join(sorted(o))}" for n, o in ESTIMATES])
def test_median_flow_matches_the_model(favlib, cuda, name, opts):
    import torch
    A, B, m32, m64 = _case(name, **opts)
    a, b = _dev(A, cuda), _dev(B, cuda)
    got_t = _flow_into_poisoned_buffers(favlib, cuda, a, b, **opts)
    got = got_t.cpu().numpy()
    assert got.shape == A.shape[:2] + (2,) and np.isfinite(got).all()
    plain = set(opts) == {"median"}
    (gate_floor if plain else gate_4e32)(got, m32, m64, f"flow with the median filter, {name} {opts}")
    assert torch.equal(favlib.flow_rgb8(a, b, **opts), got_t)                                        # the binding, fresh buffers
    assert not torch.equal(favlib.flow_rgb8(a, b, **{k: v for k, v in opts.items() if k != "median"}), got_t)
    assert not torch.equal(favlib.flow_rgb8(a, b, **dict(opts, median=8 - opts["median"])), got_t)   # 3 and 5 are two filters


# ------------------------------------------------------------------------------------------------ 3. the buffer parity
@pytest.mark.parametrize("iters,spl,warps", [(30, 6, 3), (24, 6, 3), (30, 6, 2), (24, 6, 2)])
def test_result_arrives_in_the_callers_buffer(favlib, cuda, iters, spl, warps):
    """a warp is ceil(iters / K) + 1 buffer swaps with the filter: (30, 6) gives 6 per warp, (24, 6) gives 5 -- with 3 and 2 warps the
    totals at level 0 are 18, 15, 12, 10: even and odd.  The output held NaN beforehand."""
    opts = dict(median=5, iters=iters, warps=warps)
    A, B, m32, m64 = _case("64x64", **opts)
    got = _flow_into_poisoned_buffers(favlib, cuda, _dev(A, cuda), _dev(B, cuda), sweeps_per_launch=spl, **opts).cpu().numpy()
    assert np.isfinite(got).all()
    gate_floor(got, m32, m64, f"median 5, iters {iters}, {spl} sweeps per launch, {warps} warps")


def test_median_flow_does_not_depend_on_the_temporal_blocking(favlib, cuda):
    """sweeps_per_launch 1, 4, 6, 16 at 30 sweeps: 31, 9, 6 and 3 swaps per warp, 93, 27, 18 and 9 at level 0"""
    import torch
    A, B, m32, m64 = _case("64x64", median=5)
    a, b = _dev(A, cuda), _dev(B, cuda)
    want = _flow_into_poisoned_buffers(favlib, cuda, a, b, median=5)
    for spl in (1, 4, 6, 16):
        assert torch.equal(_flow_into_poisoned_buffers(favlib, cuda, a, b, median=5, sweeps_per_launch=spl), want), spl
    for opts in (dict(median=3, smooth_eps=EPS), dict(median=5, match_beta=-1, data_term=1)):
        ref = favlib.flow_rgb8(a, b, **opts)
        for spl in (1, 16):
            assert torch.equal(favlib.flow_rgb8(a, b, sweeps_per_launch=spl, **opts), ref), (opts, spl)


# ------------------------------------------------------------------------------------------------ 4. the batch
@pytest.mark.parametrize("n", [1, 3])
def test_median_pairs_equal_single_calls(favlib, cuda, n):
    import torch
    h, w = 48, 80
    pairs = [tuple(_dev(f, cuda) for f in M.warped_pair(h, w, 40 + k)) for k in range(n)]
    prev, cur = [p for p, _ in pairs], [c for _, c in pairs]
    for opts in (dict(median=5), dict(median=3, smooth_eps=EPS, match_beta=-1)) if n == 3 else (dict(median=5),):
        bw, fw = favlib.flow_pairs(prev, cur, opts)
        for k in range(n):
            assert torch.equal(bw[k], favlib.flow_rgb8(cur[k], prev[k], **opts)), (k, opts)
            assert torch.equal(fw[k], favlib.flow_rgb8(prev[k], cur[k], **opts)), (k, opts)
        assert not torch.equal(bw[0], favlib.flow_pairs(prev, cur, {k: v for k, v in opts.items() if k != "median"})[0][0])


# ------------------------------------------------------------------------------------------------ 5. the option off
def test_ex3_entries_with_median_0_are_the_ex2_entries(favlib, cuda):
    import torch
    L = favlib.lib()
    one = lambda t: (C.c_void_p * 1)(t.data_ptr())
    void = lambda o: C.cast(C.pointer(o), C.c_void_p)
    for h, w in M.SIZES + [(64, 96)]:
        A, B = M.warped_pair(h, w, SEED)
        a, b = _dev(A, cuda), _dev(B, cuda)
        for opts in ({}, dict(smooth_eps=EPS), dict(data_term=1, smooth_eps=EPS)) + ((dict(match_beta=-1),) if h >= 32 else ()):
            ex2_o, ex3_o = favlib._flow_opts_ex2(opts), favlib._flow_opts_ex3(dict(opts, median=0))
            nb = L.fav_flow_workspace_bytes_ex2(w, h, void(ex2_o))
            assert nb == L.fav_flow_workspace_bytes_ex3(w, h, void(ex3_o)) > 0
            ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
            ex2, ex3 = torch.empty((h, w, 2), dtype=torch.float32, device=cuda), torch.empty((h, w, 2), dtype=torch.float32, device=cuda)
            favlib._check(L.fav_flow_rgb8_ex2(favlib._p(a), favlib._p(b), w, h, C.byref(ex2_o), favlib._p(ex2), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
            favlib._check(L.fav_flow_rgb8_ex3(favlib._p(a), favlib._p(b), w, h, C.byref(ex3_o), favlib._p(ex3), favlib._p(ws), C.c_size_t(nb), favlib._stream()))
            assert torch.equal(ex2, ex3) and torch.isfinite(ex2).all(), (h, w, opts)
            nbp = L.fav_flow_pairs_workspace_bytes_ex2(w, h, 1, void(ex2_o))
            assert nbp == L.fav_flow_pairs_workspace_bytes_ex3(w, h, 1, void(ex3_o)) > 0
            wsp = torch.empty(nbp, dtype=torch.uint8, device=cuda)
            o4 = [torch.empty((h, w, 2), dtype=torch.float32, device=cuda) for _ in range(4)]
            favlib._check(L.fav_flow_pairs_rgb8_ex2(one(a), one(b), 1, w, h, C.byref(ex2_o), one(o4[0]), one(o4[1]), favlib._p(wsp), C.c_size_t(nbp), favlib._stream()))
            favlib._check(L.fav_flow_pairs_rgb8_ex3(one(a), one(b), 1, w, h, C.byref(ex3_o), one(o4[2]), one(o4[3]), favlib._p(wsp), C.c_size_t(nbp), favlib._stream()))
            assert torch.equal(o4[0], o4[2]) and torch.equal(o4[1], o4[3]) and torch.equal(o4[1], ex2), (h, w, opts)


# ------------------------------------------------------------------------------------------------ 6. the stream
def test_stream_estimate_ex3_equals_the_flows_of_the_batch(favlib, cuda):
    """fav_stream_next_frame_estimate_ex3 on three 64x64 frames (the match scene's A, B, A cropped) with median 5 is
    fav_stream_next_frame_flow fed with the flows of flow_pairs(median=5): flows, mask, state and PNG bytes"""
    import torch
    h, w = 64, 64
    A, B = _inputs("match 64x96")
    frames = [_dev(np.ascontiguousarray(f[:, 16:80]), cuda) for f in (A, B, A)]
    net = favlib.Net(VID, 0)
    results = []
    for path in ("hand", "estimate", "estimate, two single calls"):
        st = favlib.Stream(net, h, w)
        st.first_frame(frames[0])
        pngs = [favlib.png_encode(None, from_stream=st)]
        for i in (1, 2):
            if path == "hand":
                bws, fws = favlib.flow_pairs([frames[i - 1]], [frames[i]], dict(median=5))
                bw, fw = bws[0], fws[0]
                st.next_frame_flow(frames[i], bw, fw, use_structure=True)
            else:
                _, _, bw, fw = st.next_frame_estimate(frames[i], frames[i - 1], use_structure=True, batched=path == "estimate", median=5)
            pngs.append(favlib.png_encode(None, from_stream=st))
        results.append((st.state().cpu().numpy(), pngs, bw.cpu().numpy(), fw.cpu().numpy(), st.last_mask().cpu().numpy()))
        st.close()
    torch.cuda.synchronize()
    for s, p, bw, fw, m in results[1:]:
        s0, p0, b0, f0, m0 = results[0]
        assert np.array_equal(bw, b0) and np.array_equal(fw, f0) and np.array_equal(m, m0) and np.array_equal(s, s0) and p == p0 and len(p) == 3
    assert not np.array_equal(results[0][2], favlib.flow_rgb8(frames[2], frames[1]).cpu().numpy())          # the option reached the estimator


# ------------------------------------------------------------------------------------------------ 7. the executable
def test_fav_flow_median_equals_the_binding(favlib, cuda, tmp_path):
    A, B = _inputs("match 64x96")
    _write_ppm(str(tmp_path / "a.ppm"), A); _write_ppm(str(tmp_path / "b.ppm"), B)
    a, b = _dev(A, cuda), _dev(B, cuda)
    for args, opts in ((["-median", "5"], dict(median=5)), (["-median", "3", "-eps", "0.3", "-match", "1"], dict(median=3, smooth_eps=0.3, match_beta=-1)),
                       (["-median", "0"], {})):
        out = tmp_path / "out.flo"
        _run([os.path.join(BIN, "fav_flow")] + args + [str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm"), str(out)])
        want = favlib.flow_rgb8(a, b, **opts).cpu().numpy()
        payload = open(out, "rb").read()
        assert payload[:4] == b"PIEH" and payload[12:] == want.tobytes(), args
