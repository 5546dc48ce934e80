"""Observe ONE layer of a network through the public API, to ~1e-6: everything behind the layer under test is made transparent by the
choice of its weights ("Per-kernel parity through an identity tail").

For the layer under test L (item `index_of_L` of the arch string `<prefix>,L,c9s1-3`):

  * the norm directly behind L gets gamma = 1 and beta = B -- an nn.InstanceNormalization ("stats" variant: the convolution together with
    the statistics its kernel's epilogue writes) or an evaluate-mode nn.SpatialBatchNormalization with mean 0 and var 1 - eps ("raw"
    variant: a fixed shift, so the bias is observed too).  B makes every pre-ReLU value of the float64 reference >= 1: the ReLU is the identity;
  * the last c9s1-3 layer (the observer) has zero bias and zero taps except the centre one, which is +-2^-k on a disjoint group of at most
    GROUP_MAX of L's channels per output channel, signs alternating inside a group.  2^-k keeps |tanh argument| <= 0.5 in the float64 reference;
    y = atanh(out / 150) * 2^k recovers the signed group sums.  Three groups per checkpoint: ceil(C / (3 * GROUP_MAX)) checkpoints cover all channels;
  * a residual block (L = R<n>) ends in InstanceNorm + join with no ReLU: the observer sees skip + IN(branch) as it is, gamma / beta random;
  * the last layer itself (index_of_L = the last item) is observed directly: its weights are scaled by a power of two so that the
    reference's tanh argument stays below 0.5, and atanh(out / 150) is compared.

The reference is a float64 model of the layer list (torch on the CPU), run on extract_layers() of the very checkpoint the GPU loads.  Nothing
in here calls the library under test."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from fav_amd import t7

TOL_RAW = 2e-4        # single convolution: 2e-4 * output scale     (tests/test_gpu_parity.py, header)
TOL_STATS = 5e-4      # convolution + InstanceNorm: 5e-4 * output scale
TANH_MUL = 150.0
GROUP_MAX = 8         # (at most 16 would do: with 8 a pixel moved by 1e-2 sigma is twice the tolerance instead of barely above it)
GROUPS_PER_PASS = 3   # the observer is the network's last layer: three output channels


# ------------------------------------------------------------------------------------------------ float64 model
def instnorm64(x, gamma, beta, eps):
    mean = x.mean(dim=(1, 2), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(1, 2), keepdim=True)           # biased
    return (x - mean) / torch.sqrt(var + eps) * gamma[:, None, None] + beta[:, None, None]


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def forward64(layers, x, trace=None, convs=None, conv_ins=None):
    """the layer list of t7.extract_layers in float64; x: torch [C][H][W] float64.  trace: (type, tensor) per top-level layer;
    convs: the raw output of every convolution, residual branches included, in the network's convolution order; conv_ins: what each of
    them reads (before its own zero padding), in the same order"""
    for L in layers:
        t = L["type"]
        if conv_ins is not None and t in ("conv", "fullconv"): conv_ins.append(x)
        if t == "pad":
            x = F.pad(x[None], (L["l"], L["r"], L["t"], L["b"]), mode="replicate" if L.get("mode") == "replicate" else "reflect")[0]
        elif t == "conv":
            x = F.conv2d(x[None], _t64(L["w"]), None if L["b"] is None else _t64(L["b"]), stride=L["stride"], padding=L["pad"])[0]
        elif t == "fullconv":
            x = F.conv_transpose2d(x[None], _t64(L["w"]), None if L["b"] is None else _t64(L["b"]), stride=L["stride"], padding=L["pad"],
                                   output_padding=L["adj"])[0]
        elif t == "bn":
            s = _t64(L["gamma"]) / torch.sqrt(_t64(L["var"]) + L["eps"])
            x = (x - _t64(L["mean"])[:, None, None]) * s[:, None, None] + _t64(L["beta"])[:, None, None]
        elif t == "in":
            x = instnorm64(x, _t64(L["gamma"]), _t64(L["beta"]), L["eps"])
        elif t == "relu":
            x = torch.clamp(x, min=0)
        elif t == "res":
            y = forward64(L["block"], x, convs=convs, conv_ins=conv_ins)
            s = L["shave"]
            x = y + (x[:, s:x.shape[1] - s, s:x.shape[2] - s] if s else x)
        elif t == "up":
            x = x.repeat_interleave(L["s"], dim=1).repeat_interleave(L["s"], dim=2)
        elif t == "tanh":
            x = torch.tanh(x)
        elif t == "mul":
            x = x * L["k"]
        elif t == "identity":
            pass
        else:
            raise ValueError(t)
        if convs is not None and t in ("conv", "fullconv"): convs.append(x)
        if trace is not None: trace.append((t, x))
    return x


def _last_conv(layers):
    return max(i for i, L in enumerate(layers) if L["type"] == "conv")


def observed_index(types):
    """index (in a top-level list of layer types) of the tensor the observer reads: what comes out in front of the last convolution,
    a padding layer of the observer's own not counted"""
    j = max(i for i, t in enumerate(types) if t == "conv") - 1
    if types[j] == "pad": j -= 1
    return j


def reference_parts(layers, x):
    """float64: (the observed tensor [C][H][W], the pre-ReLU tensor of the norm behind L or None, the tanh argument [3][H][W])"""
    tr = []
    forward64(layers, _t64(x), tr)
    types = [t for t, _ in tr]
    j = observed_index(types)
    pre = tr[j - 1][1] if types[j] == "relu" else None
    return tr[j][1].numpy(), (None if pre is None else pre.numpy()), tr[_last_conv(layers)][1].numpy()


# ------------------------------------------------------------------------------------------------ the observer
def make_table(channels, k):
    """disjoint groups of at most GROUP_MAX consecutive channels, alternating signs inside a group, GROUPS_PER_PASS groups per pass"""
    passes_n = -(-channels // (GROUP_MAX * GROUPS_PER_PASS))
    assert channels % 2 == 0
    # whole PAIRS of channels per group: an even group size, so that the B offsets cancel and do not widen max |ref|
    groups = [g.reshape(-1) for g in np.array_split(np.arange(channels).reshape(-1, 2), passes_n * GROUPS_PER_PASS)]
    assert all(0 < len(g) <= GROUP_MAX for g in groups)
    passes = []
    for p in range(passes_n):
        passes.append([(g, np.where(np.arange(len(g)) % 2 == 0, 1.0, -1.0)) for g in groups[p * GROUPS_PER_PASS:(p + 1) * GROUPS_PER_PASS]])
    return {"k": int(k), "passes": passes, "channels": channels}


def sums_of(y, table):
    """signed group sums of a [C][H][W] tensor, float64: [groups][H][W]"""
    if table["passes"] is None: return np.asarray(y, np.float64)
    y = np.asarray(y, np.float64)
    return np.stack([np.tensordot(s, y[g], axes=(0, 0)) for p in table["passes"] for g, s in p])


def observer_weights(table, p):
    w = np.zeros((GROUPS_PER_PASS, table["channels"], 9, 9), np.float32)
    for j, (g, s) in enumerate(table["passes"][p]):
        w[j, g, 4, 4] = (s * 2.0 ** -table["k"]).astype(np.float32)
    return w


def observe(out3_list, table):
    """the network outputs of all passes ([3][H][W], the reference's 150 * tanh space) -> what the observer saw, float64"""
    v = np.concatenate([np.arctanh(np.asarray(o, np.float64) / TANH_MUL) for o in out3_list])
    return v * 2.0 ** table["k"]


def reference_sums(layers, x, table):
    """float64 model of the checkpoint's own layers: the signed sums the observer should see (direct mode: the last layer's output)"""
    y, _, arg = reference_parts(layers, x)
    if table["passes"] is None: return arg
    return sums_of(y, table)


def assert_close(got, ref, tol, what=""):
    """max |got - ref| <= tol * max(1, max |ref|) over EVERY observed element; returns the normalised error"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite observed values" % what
    err = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
    assert err <= tol, "%s: max normalised error %.3e > %.1e (max |ref| %.3f)" % (what, err, tol, np.abs(ref).max())
    return err


# ------------------------------------------------------------------------------------------------ geometry
def _item_out(v, h, down_shave):
    c0 = v[0]
    if c0 == "c": f, s = int(v[1]), int(v[3]); return (h + 2 * ((f - 1) // 2) - f) // s + 1
    if c0 == "d": return (h + 2 - 3) // 2 + 1
    if c0 == "U": return h * int(v[1:])
    if c0 == "u": return 2 * h
    if c0 == "f": f, s = int(v[1]), int(v[3]); return (h - 1) * s - 2 * ((f - 1) // 2) + f + s - 1
    if c0 in "RC": return h - 4 if down_shave else h
    raise ValueError(v)


def front_pad(arch, padding_type="reflect-start", insert_pad=True):
    """the lazily inserted leading reflection padding, as t7.build_model sums it"""
    lost, down = 0, 1
    for v in arch.split(","):
        if v[0] == "c": down *= int(v[3])
        elif v[0] == "d": down *= 2
        elif v[0] == "U": down = max(down // int(v[1:]), 1)
        elif v[0] == "u": down //= 2
        elif v[0] == "f": down = max(down // int(v[3]), 1)
        elif v[0] in "RC": lost += 2 * down
    return lost if insert_pad and lost and padding_type == "reflect-start" else 0


def input_size(arch, index_of_L, want, padding_type="reflect-start", **_):
    """the smallest input extent for which item index_of_L of the arch string puts out `want` pixels (one axis)"""
    items = arch.split(",")
    p = front_pad(arch, padding_type)
    for h in range(max(1, p + 1), 400):
        o = h + 2 * p
        for v in items[:index_of_L + 1]:
            o = _item_out(v, o, padding_type in ("none", "reflect-start"))
            if o < 1: break
        if o == want: return h
    raise ValueError("no input size gives %d behind item %d of %s" % (want, index_of_L, arch))


def conv_index(arch, index_of_L):
    """index of L's first convolution in the network's convolution order (what fav_net's profile is indexed by)"""
    return sum(2 if v[0] in "RC" else (0 if v[0] == "U" else 1) for v in arch.split(",")[:index_of_L])


# ------------------------------------------------------------------------------------------------ channel regimes
# IN(conv) does not change (up to eps) under a per-output-channel affine change of the convolution, so a probe's output channels can be
# put where InstanceNorm statistics go wrong without touching what the observer needs (tests/test_gpu_stats_edges.py).  Channel c of
# L gets regime REGIMES[c % 6]: every observer group of 8 consecutive channels holds all six, "plain" as the control.
#   plain    as drawn: |mean| <~ sigma, sigma of order 1-10
#   offset+- bias +- 2^j, 2^j ~ 2^OFFSET_LOG2 x sigma: a one-pass fp32 variance is off by percent, a miscounted tile moves the mean by many sigma
#   big      filters and bias x 2^m, channel RMS in [2^10, 2^11): a full 16 x 16 unit's sum of squares is beyond 2^28
#   small    x 2^-m, sigma in [2^-9, 2^-8): the variance is comparable to eps = 1e-5
#   flat     filters zero, bias 0.5 / 0 by turns: the variance is exactly zero and the reference output exactly beta.  (|bias| <= 1: what
#            is observed is the fp32 rounding of the mean / sqrt(eps))
REGIMES = ("plain", "offset+", "big", "offset-", "small", "flat")
OFFSET_LOG2 = 9       # offset / sigma = 2^9 (tests/test_cpu_stats_edges.py: the fp32 oracle stays within a quarter of the bound at this ratio)


def regime_of(c, names=REGIMES):
    return names[c % len(names)]


def _conv_modules(m, out=None):
    """every convolution module below m, in extract_layers' order (a residual branch in front of what follows the block)"""
    out = [] if out is None else out
    for q in m.fields.get("modules", []):
        if q.cls in ("nn.SpatialConvolution", "nn.SpatialFullConvolution"): out.append(q)
        elif q.cls in ("nn.Sequential", "nn.ConcatTable"): _conv_modules(q, out)
    return out


def _stats(z):
    z = np.asarray(z, np.float64).reshape(z.shape[0], -1)
    return z.std(axis=1), np.sqrt((z * z).mean(axis=1))


def _conv_regimes(mod, z):
    """put the output channels of one convolution module into their regimes; z: its float64 output [C][H][W] as the weights stand"""
    w, b = mod.fields["weight"], mod.fields["bias"]
    axis = 1 if mod.cls == "nn.SpatialFullConvolution" else 0              # [cin][cout][k][k] there
    sd, rms = _stats(z)
    flats = 0
    for c in range(z.shape[0]):
        r = regime_of(c)
        sl = tuple(c if a == axis else slice(None) for a in range(4))
        if r in ("offset+", "offset-"):
            b[c] = np.float32(b[c]) + np.float32((1.0 if r == "offset+" else -1.0) * 2.0 ** (round(math.log2(sd[c])) + OFFSET_LOG2))
        elif r in ("big", "small"):
            m = 10 - math.floor(math.log2(rms[c])) if r == "big" else -9 - math.floor(math.log2(sd[c]))
            w[sl] = w[sl] * np.float32(2.0 ** m); b[c] = b[c] * np.float32(2.0 ** m)       # exact: powers of two
        elif r == "flat":
            w[sl] = 0; b[c] = 0.5 if flats % 2 == 0 else 0.0; flats += 1


# L = U<n> carries its own InstanceNorm + ReLU and has no weights: the regimes of the tensor whose statistics are taken come from the
# norm(s) in front, with powers of two as gamma.  What each construction can reach:
#   behind `c..., U<n>` (stats_kernel on a pending InstanceNorm + ReLU): the prefix norm gets gamma = 2^m, beta >= gamma x (1 - min of
#     the normalised channel), so that the ReLU stays the identity -- the mean is therefore at least ~4 sigma everywhere.  plain (gamma 1,
#     beta B0 = that minimum), offset+ (beta 2^9), big (gamma 2^m with RMS in [2^10, 2^11)), small (gamma 2^-9), flat (gamma 0, beta 0.5 / 0).
#     offset- is out of reach: a negative mean would not pass the ReLU.
#   behind `R<n>, U<n>` (res_add_stats_kernel: z = skip + IN(branch)): the branch's last norm -- plain (as drawn), offset+ / offset- (gamma 1,
#     beta +- 2^j ~ 2^9 sigma_z), big (gamma 2^10, beta 2^9).  small and flat need the skip term small / constant as well: the prefix norm of
#     these channels gets gamma 2^-9 / 0 too (small: gamma 2^-9 on both; flat: gamma 0 on both, beta 0.5 / 0 on the branch's norm).
U_STATS_REGIMES = ("plain", "offset+", "big", "small", "flat")


def _norm_regimes(model, arch, index_of_L, x, kw, tmp):
    mods = model.fields["modules"]
    up_i = [i for i, m in enumerate(mods) if m.cls == "nn.SpatialUpSamplingNearest"][-1]
    join = mods[up_i - 1].cls == "nn.Sequential"
    prefix = mods[up_i - 3 if join else up_i - 2]
    assert prefix.cls == "nn.InstanceNormalization", prefix.cls
    C = int(prefix.fields["nOutput"])
    g0, b0 = np.ones((C,), np.float32), np.zeros((C,), np.float32)
    prefix.fields["weight"], prefix.fields["bias"] = g0, b0

    def trace():
        tr = []
        forward64(_write(tmp, model, arch, kw), _t64(x), tr)
        os.remove(tmp)
        u = max(i for i, (t, _) in enumerate(tr) if t == "up")
        return tr, u

    tr, u = trace()
    nhat = tr[u - (3 if join else 2)][1].numpy()                   # the prefix norm's output at gamma 1, beta 0
    assert tr[u - (3 if join else 2)][0] == "in"
    B0 = np.ceil(1.0 - nhat.reshape(C, -1).min(axis=1))             # gamma x (nhat + B0) >= gamma: the ReLU is the identity
    if not join:
        flats = 0
        for c in range(C):
            r = regime_of(c, U_STATS_REGIMES)
            if r == "plain": b0[c] = B0[c]
            elif r == "offset+": b0[c] = 2.0 ** OFFSET_LOG2
            elif r == "big":
                g0[c] = 2.0 ** (10 - math.floor(math.log2(math.sqrt(1.0 + B0[c] ** 2)))); b0[c] = g0[c] * B0[c]
            elif r == "small": g0[c] = 2.0 ** -9; b0[c] = g0[c] * B0[c]
            else: g0[c] = 0.0; b0[c] = 0.5 if flats % 2 == 0 else 0.0; flats += 1
        return [regime_of(c, U_STATS_REGIMES) for c in range(C)]
    last = mods[up_i - 1].fields["modules"][0].fields["modules"][0].fields["modules"][-1]      # Sequential(ConcatTable(branch, skip), CAddTable)
    assert last.cls == "nn.InstanceNormalization", last.cls
    g1, b1 = last.fields["weight"], last.fields["bias"]
    b0[:] = B0
    flats = 0
    for c in range(C):
        r = regime_of(c)
        if r in ("offset+", "offset-"): g1[c] = 1.0
        elif r == "big": g1[c] = 2.0 ** 10; b1[c] = 2.0 ** 9
        elif r == "small": g1[c] = 2.0 ** -9; g0[c] = 2.0 ** -9; b0[c] = g0[c] * B0[c]
        elif r == "flat": g1[c] = 0.0; g0[c] = 0.0; b0[c] = 0.0; b1[c] = 0.5 if flats % 2 == 0 else 0.0; flats += 1
    tr, u = trace()
    sd, _ = _stats(tr[u - 1][1].numpy())                            # the joined tensor, the offsets still missing
    for c in range(C):
        r = regime_of(c)
        if r in ("offset+", "offset-"): b1[c] = (1.0 if r == "offset+" else -1.0) * 2.0 ** (round(math.log2(sd[c])) + OFFSET_LOG2)
    return [regime_of(c) for c in range(C)]


# ------------------------------------------------------------------------------------------------ bf16-exact probes
# fav_net_set_precision(1) runs the 3x3 stride-1 layers on conv3_halo_bf16_kernel: activations (after the pending norm / ReLU stages) and
# weights rounded to bf16, fp32 accumulation.  A probe whose rounding is the IDENTITY holds that kernel to the float64 convolution at the
# ordinary per-kernel tolerances -- a bf16 x bf16 product is exact in fp32, what remains is the accumulation:
#   * input: seeded integers in [-8, 8];
#   * every convolution in front of L's last one (the first layer; a block's first convolution): two taps of +-1 per filter and an
#     integer bias in [-2, 2] -- its float64 output is an integer or a dyadic of few bits, and fp32 arithmetic on it is exact;
#   * every norm in front of L: evaluate-mode BatchNorm (a pending stage, net.cpp `case L_BN`) with mean 0, var 1 - eps, per channel
#     gamma from BF16_SCALES (rotating, so that channels c and c + 32 differ) and an integer beta that centres the channel -- chosen so
#     that relu(gamma z + beta) is bf16-representable everywhere (asserted: probe_checkpoints, is_bf16).  The library's fp32 scale is
#     gamma / sqrt(fl32(1 - eps) + eps) = gamma (1 - 1.5e-8), which rounds to gamma itself; the reference runs these norms with the
#     intended numbers (var 1, eps 0).  What the kernel rounds on the GPU then differs from a bf16 number by a few fp32 ulps at most
#     (the scale to within an ulp, a producer kernel's own rounding): 2^-22 relative, against half a bf16 ulp = 2^-9 -- the kernel's own
#     round-to-nearest absorbs it, no rounding can flip (a value that is exactly 0 in the reference may come out ~1e-5 instead of 0:
#     that is an absolute error of 1e-5 x a weight, far below the bound);
#   * the norm behind L: BatchNorm ("raw") or InstanceNorm with gamma 1, beta B ("stats": the bf16 kernel's partials / counts epilogue
#     through in_finalize) -- swapped into the model tree, so the stats variant is a mixed checkpoint;
#   * the weights of L's last convolution: as drawn, NOT bf16 numbers.  The reference convolves with bf16_round(w) -- the host's
#     round-to-nearest-even copy (net_model.cpp, wgt16) is under test, and the probe fails if the fp32 kernel ran instead.
BF16_SCALES = (0.5, -1.0, 2.0, 1.5, -0.5, 1.0, -2.0)


def is_bf16(a):
    """every value of a float64 array is a bf16 number"""
    import oracle
    a = np.asarray(a, np.float64)
    f = a.astype(np.float32)
    return bool(np.all(f.astype(np.float64) == a) and np.all(oracle.bf16_round(f) == f))


def conv_layers(layers, out=None):
    """the convolution layers of an extract_layers list in the network's convolution order (forward64's `convs`)"""
    out = [] if out is None else out
    for L in layers:
        if L["type"] in ("conv", "fullconv"): out.append(L)
        elif L["type"] == "res": conv_layers(L["block"], out)
    return out


def front_norms(layers, conv0, n_convs):
    """the BatchNorm layers whose output a convolution under test reads (through ReLU / upsampling / padding): every top-level one in
    front of L, and the one between the two convolutions of a block"""
    first = conv_layers(layers)[conv0]
    out = []
    for L in layers:
        if L is first: return out
        if L["type"] == "bn": out.append(L)
        if L["type"] == "res" and any(q is first for q in L["block"]):
            assert n_convs == 2
            return out + [q for q in L["block"][:-1] if q["type"] == "bn"]
    raise ValueError("convolution %d not found" % conv0)


def bf16_reference_layers(layers, conv0, n_convs):
    """what the float64 reference of a bf16 probe runs: the checkpoint's layers with the weights of L's convolutions rounded to bf16
    (nearest even) and the norms in front of them with the intended scale (var 1, eps 0 instead of var fl32(1 - eps), eps)"""
    import copy
    import oracle
    ls = copy.deepcopy(layers)
    for L in conv_layers(ls)[conv0:conv0 + n_convs]: L["w"] = oracle.bf16_round(L["w"])
    for L in front_norms(ls, conv0, n_convs):
        assert np.all(L["mean"] == 0) and np.all(L["var"] == np.float32(1.0 - L["eps"]))
        L["var"] = np.ones_like(L["var"]); L["eps"] = 0.0
    return ls


def bf16_conv_inputs(layers, x):
    """float64: what every convolution reads, in the network's convolution order"""
    ins = []
    forward64(layers, _t64(x), conv_ins=ins)
    return [a.numpy() for a in ins]


def _sparse_conv(mod, rng):
    w = np.zeros_like(mod.fields["weight"])
    cout, cin, k, _ = w.shape
    for o in range(cout):
        for pos in rng.choice(cin * k * k, size=2, replace=False):
            w[o].reshape(-1)[pos] = rng.choice((-1.0, 1.0))
    mod.fields["weight"] = w
    mod.fields["bias"] = rng.integers(-2, 3, size=cout).astype(np.float32)


def _fit_norm(bn, z):
    """gamma / beta of an evaluate-mode BatchNorm in front of L; z: float64 [C][H][W], what it reads"""
    C = z.shape[0]
    assert bn.cls == "nn.SpatialBatchNormalization" and bn.fields["weight"].shape == (C,)
    g, b = np.zeros((C,), np.float32), np.zeros((C,), np.float32)
    for c in range(C):
        for t in range(len(BF16_SCALES)):
            s = BF16_SCALES[(c + t) % len(BF16_SCALES)]
            sh = float(c % 5 - 1 - round(s * float(np.median(z[c]))))
            v = np.maximum(z[c] * s + sh, 0.0)
            if is_bf16(v) and v.max() > 0: break
        else:
            raise AssertionError("no scale keeps channel %d bf16-representable" % c)
        g[c], b[c] = s, sh
    bn.fields["weight"], bn.fields["bias"] = g, b
    bn.fields["running_mean"] = np.zeros((C,), np.float32)
    bn.fields["running_var"] = np.full((C,), 1.0 - float(bn.fields["eps"]), np.float32)


def _bf16_front(model, arch, index_of_L, variant, seed, x_shape, kw, tmp):
    """make everything in front of L's last convolution bf16-exact (see above) and put the norm `variant` asks for behind L; returns the input"""
    rng = np.random.default_rng(seed + 2000)
    x = rng.integers(-8, 9, size=x_shape).astype(np.float32)
    mods = model.fields["modules"]
    c0 = conv_index(arch, index_of_L)
    block = arch.split(",")[index_of_L][0] in "RC"
    cm = _conv_modules(model)
    assert cm[c0].fields["kW"] == 3 and cm[c0].fields["dW"] == 1, "bf16 probes are for the 3x3 stride-1 layers"
    for m in cm[:c0 + (1 if block else 0)]: _sparse_conv(m, rng)
    iL = next(i for i, m in enumerate(mods) if m is cm[c0] or (m.cls == "nn.Sequential" and any(q is cm[c0] for q in _conv_modules(m))))
    inner = mods[iL].fields["modules"][0].fields["modules"][0].fields["modules"] if block else None      # Sequential(ConcatTable(branch, skip), CAddTable)
    # the norm behind L
    holder, at = (inner, len(inner) - 1) if block else (mods, iL + 1)
    assert holder[at].cls == "nn.SpatialBatchNormalization", holder[at].cls
    C = int(cm[c0].fields["nOutputPlane"])
    if variant == "stats": holder[at] = t7._inorm(rng, C)
    if block:
        # behind a join the observer sees skip + norm(branch), the skip of order 10: the branch is made to dominate max |ref| -- its
        # InstanceNorm with gamma 32, beta 0 (sigma 32), its BatchNorm the identity (the raw convolution, sigma of order 30, bias included)
        f = holder[at].fields
        f["weight"] = np.full((C,), 32.0 if variant == "stats" else 1.0, np.float32); f["bias"] = np.zeros((C,), np.float32)
        if variant == "raw": f["running_mean"] = np.zeros((C,), np.float32); f["running_var"] = np.full((C,), 1.0 - float(f["eps"]), np.float32)
    # the norms in front, in the network's order: each is fitted to the float64 tensor it reads with the earlier ones in place
    fits = [(mods[i], ("top", i)) for i in range(iL) if mods[i].cls == "nn.SpatialBatchNormalization"]
    if block: fits += [(m, ("conv", c0)) for m in inner[:-1] if m.cls == "nn.SpatialBatchNormalization"]
    assert fits
    done = 0
    for bn, (kind, i) in fits:
        tr, convs = [], []
        layers = _write(tmp, model, arch, kw)
        os.remove(tmp)
        for L in (front_norms(layers, c0, 2 if block else 1)[:done]): L["var"] = np.ones_like(L["var"]); L["eps"] = 0.0      # (as the reference runs them)
        done += 1
        forward64(layers, _t64(x), tr, convs)
        if kind == "top": assert tr[i][0] == "bn", tr[i][0]
        _fit_norm(bn, (tr[i - 1][1] if kind == "top" else convs[i]).numpy())
    return x


# ------------------------------------------------------------------------------------------------ checkpoints
class Probe:
    pass


def _write(path, model, arch, kw):
    t7.write_checkpoint(path, {"opt": {"arch": arch, "padding_type": kw.get("padding_type", "reflect-start"),
                                       "use_instance_norm": 1, "tanh_constant": TANH_MUL},
                               "train_loss_history": {}, "val_loss_history": {}, "iter": 0, "model": model})
    return t7.extract_layers(t7.load(path)["model"])


def probe_checkpoints(arch, index_of_L, variant, seed, hw, out_dir, regimes=False, bf16=False, **build_kw):
    """Checkpoints (one per pass) that observe item index_of_L of `arch` on a seeded random input of hw = (H, W), and the observer's
    group / sign table.  variant: "stats" (InstanceNorm everywhere) or "raw" (evaluate-mode BatchNorm everywhere).
    bf16: the probe for the bf16-operand fast mode ("bf16-exact probes" below) -- BatchNorm everywhere but behind L, where `variant`
    decides; the Probe then carries ref_layers, the layer list the float64 reference runs.
    regimes ("stats" only: raw has no statistics): the output channels of L -- of both convolutions of an R<n> item -- by turns in the
    regimes of REGIMES above; sigma and RMS of a channel are those of the float64 reference as the weights stand when its convolution
    is changed (the block's second convolution: behind the changed first).  B and k come from the changed checkpoint, as always.
    Returns a Probe: paths, table, x [cin][H][W] float32, layers (extract_layers of the first path), B, direct."""
    assert variant in ("stats", "raw")
    items = arch.split(",")
    direct = index_of_L == len(items) - 1
    assert direct or items[index_of_L + 1:] == ["c9s1-3"], "the observer is one c9s1-3 item directly behind L"
    kw = dict(build_kw, use_instance_norm=(variant == "stats" and not bf16))
    model = t7.build_model(arch, seed, **kw)
    mods = model.fields["modules"]
    cin = kw.get("in_channels", 7)
    # N(0, 60) like the network tests; N(0, 1) where nothing normalises (BatchNorm with random running statistics): activations of order 1,
    # so that a bias of +-0.1 is well above 2e-4 of the observed scale
    x = (np.random.default_rng(seed + 1000).standard_normal((cin, hw[0], hw[1])) * (60 if variant == "stats" else 1)).astype(np.float32)
    obs_i = max(i for i, m in enumerate(mods) if m.cls == "nn.SpatialConvolution")
    obs = mods[obs_i]
    tag = "%s_%d_%s%s_%d_%dx%d" % (arch.replace(",", "_"), index_of_L, variant, "_regimes" if regimes else ("_bf16" if bf16 else ""), seed, hw[0], hw[1])
    base = os.path.join(str(out_dir), tag)
    n_convs = 2 if items[index_of_L][0] in "RC" else 1
    # what the float64 reference runs: the checkpoint's own layers, or (bf16) those with L's weights rounded and the norms in front exact
    ref_of = (lambda ls: bf16_reference_layers(ls, conv_index(arch, index_of_L), n_convs)) if bf16 else (lambda ls: ls)
    if bf16:
        assert not regimes and not direct, "bf16 probes: a 3x3 layer behind an observer, no regimes"
        x = _bf16_front(model, arch, index_of_L, variant, seed, x.shape, kw, base + "_tmp.t7")
    pr = Probe()
    pr.x, pr.direct, pr.B, pr.arch, pr.variant = x, direct, 0.0, arch, variant

    if direct:
        layers = _write(base + "_tmp.t7", model, arch, kw)
        arg = reference_parts(layers, x)[2]
        m = max(0, math.ceil(math.log2(float(np.abs(arg).max()) / 0.5)))           # scaling by 2^-m is exact: weights stay fp32 numbers
        obs.fields["weight"] = (obs.fields["weight"] * np.float32(2.0 ** -m)).astype(np.float32)
        obs.fields["bias"] = (obs.fields["bias"] * np.float32(2.0 ** -m)).astype(np.float32)
        pr.table = {"k": 0, "passes": None, "channels": 3}
        pr.paths = [base + ".t7"]
        pr.layers = _write(pr.paths[0], model, arch, kw)
        os.remove(base + "_tmp.t7")
        return pr

    # the norm directly behind L: [norm, ReLU, (the observer's own padding layer), observer]; nothing to set behind a residual block
    j = obs_i - 1
    if mods[j].cls in ("nn.SpatialReflectionPadding", "nn.SpatialReplicationPadding"): j -= 1
    norm = None
    if mods[j].cls == "nn.ReLU":
        norm = mods[j - 1]
        assert norm.cls == ("nn.InstanceNormalization" if variant == "stats" else "nn.SpatialBatchNormalization"), norm.cls
    else:
        assert mods[j].cls == "nn.Sequential", mods[j].cls
    C = int(obs.fields["nInputPlane"])

    def set_norm(B):
        if norm is None: return
        norm.fields["weight"] = np.ones((C,), np.float32)
        norm.fields["bias"] = np.full((C,), B, np.float32)
        if variant == "raw":
            norm.fields["running_mean"] = np.zeros((C,), np.float32)
            norm.fields["running_var"] = np.full((C,), 1.0 - float(norm.fields["eps"]), np.float32)

    obs.fields["bias"] = np.zeros((3,), np.float32)
    obs.fields["weight"] = np.zeros((3, C, 9, 9), np.float32)
    set_norm(0.0)
    pr.regimes = None
    if regimes:
        assert variant == "stats", "regimes: the statistics variant only"
        if items[index_of_L][0] == "U":
            pr.regimes = _norm_regimes(model, arch, index_of_L, x, kw, base + "_tmp.t7")
        else:
            c0 = conv_index(arch, index_of_L)
            for i in range(2 if items[index_of_L][0] in "RC" else 1):
                convs = []
                forward64(_write(base + "_tmp.t7", model, arch, kw), _t64(x), convs=convs)
                os.remove(base + "_tmp.t7")
                _conv_regimes(_conv_modules(model)[c0 + i], convs[c0 + i].numpy())
            pr.regimes = [regime_of(c) for c in range(C)]
    layers = _write(base + "_tmp.t7", model, arch, kw)
    y0, pre0, _ = reference_parts(ref_of(layers), x)
    os.remove(base + "_tmp.t7")
    if norm is not None:
        pr.B = float(math.ceil(1.5 - float(pre0.min())))        # min pre-ReLU value >= 1.5 in the reference: the ReLU is the identity on the GPU too
        set_norm(pr.B)
    # k from the reference at this B (the offsets cancel in a group of even size and count once in an odd one)
    s0 = sums_of(y0 if norm is None else pre0 + pr.B, make_table(C, 0))
    k = max(0, math.ceil(math.log2(float(np.abs(s0).max()) * 1.05 / 0.5)))
    pr.table = make_table(C, k)
    pr.paths = []
    for p in range(len(pr.table["passes"])):
        obs.fields["weight"] = observer_weights(pr.table, p)
        pr.paths.append("%s_p%d.t7" % (base, p))
        ls = _write(pr.paths[-1], model, arch, kw)
        if p == 0: pr.layers = ls
    if bf16:
        pr.ref_layers = ref_of(pr.layers)
        c0 = conv_index(arch, index_of_L)
        for a in bf16_conv_inputs(pr.ref_layers, x)[c0:c0 + n_convs]:      # a badly built probe fails here, before a GPU sees it
            assert is_bf16(a), "bf16 probe %s: a tensor in front of L is not bf16-representable in the reference" % tag
    return pr


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_layer_parity.py
def _case(name, arch, index_of_L, out, ids, poison=False, ids_raw=None, **kw):
    return {"name": name, "arch": arch, "L": index_of_L, "out": out, "ids": ids, "ids_raw": ids_raw or ids, "poison": poison, "kw": kw}


# name, arch, item under test, ITS output size, the profile ids its convolutions must report (fav_internal.h, enum ConvKernel).  Sizes per
# kernel, from its *_tiles() function: less than one tile both ways | exactly one tile | whole tiles plus one row and one column
CASES = [
    # CK_FIRST2D, 16 x 32 tiles: 7 and 3 input channels; 32, 64, 96 filters (96 runs as 128 with zero filters)
    _case("first2d_7_32_small", "c9s1-32,c9s1-3", 0, (9, 20), [16], poison=True),
    _case("first2d_7_32_tile", "c9s1-32,c9s1-3", 0, (16, 32), [16]),
    _case("first2d_7_32_ragged", "c9s1-32,c9s1-3", 0, (33, 65), [16]),
    _case("first2d_3_64", "c9s1-64,c9s1-3", 0, (17, 33), [16], in_channels=3),
    _case("first2d_7_96", "c9s1-96,c9s1-3", 0, (17, 33), [16]),
    # CK_S2W, 4 x 32 tiles (64 filters) | 3 x 32 (128-filter groups)
    _case("s2w_32_64_small", "c9s1-32,d64,c9s1-3", 1, (3, 20), [764], poison=True),
    _case("s2w_32_64_tile", "c9s1-32,d64,c9s1-3", 1, (4, 32), [764]),
    _case("s2w_32_64_ragged", "c9s1-32,d64,c9s1-3", 1, (9, 65), [764]),
    _case("s2w_64_128", "c9s1-64,d128,c9s1-3", 1, (7, 33), [828]),
    _case("s2w_128_256", "c9s1-128,d256,c9s1-3", 1, (4, 33), [956]),
    # CK_WINO4, 16 x 16 units.  R<n>: both convolutions of a block -- the first one's InstanceNorm is consumed as accumulators by the
    # second, the second one's by the join; c3s1-128 behind a padding layer: 16 / 48 (runs as 64) / 64 input channels, with a pending
    # norm, and without one behind a join
    _case("wino4_R128_small", "c9s1-128,R128,c9s1-3", 1, (9, 11), [728, 728], poison=True),
    _case("wino4_R128_tile", "c9s1-128,R128,c9s1-3", 1, (16, 16), [728, 728]),
    _case("wino4_R128_ragged", "c9s1-128,R128,c9s1-3", 1, (33, 33), [728, 728]),
    _case("wino4_R256", "c9s1-256,R256,c9s1-3", 1, (17, 17), [856, 856]),
    _case("wino4_cin16", "c9s1-16,c3s1-128,c9s1-3", 1, (17, 17), [728], padding_type="reflect"),
    _case("wino4_cin48", "c9s1-48,c3s1-128,c9s1-3", 1, (17, 17), [728], padding_type="reflect"),
    _case("wino4_cin64", "c9s1-64,c3s1-128,c9s1-3", 1, (17, 17), [728], padding_type="replicate"),
    _case("wino4_no_pending_norm", "c9s1-128,R128,c3s1-128,c9s1-3", 2, (17, 17), [728], padding_type="reflect"),
    # CK_UP2 behind a join (R64, U2), tiles of 4 x 32 physical = 8 x 64 output pixels
    _case("up2_64_small", "c9s1-64,R64,U2,c3s1-64,c9s1-3", 3, (6, 40), [564], poison=True),
    _case("up2_64_tile", "c9s1-64,R64,U2,c3s1-64,c9s1-3", 3, (8, 64), [564]),
    _case("up2_64_ragged", "c9s1-64,R64,U2,c3s1-64,c9s1-3", 3, (18, 130), [564]),
    _case("up2_128", "c9s1-64,R64,U2,c3s1-128,c9s1-3", 3, (10, 66), [628]),
    _case("up2_256", "c9s1-64,R64,U2,c3s1-256,c9s1-3", 3, (10, 66), [756]),
    # CK_HALO3, 8 x 32 tiles and 16 x 16 ones on a ragged right edge of at most 16 columns.  The three pad_* cases put a padding layer in
    # front of L (padding_type reflect / replicate): the library runs it as the element kernel pad_nhwc.  Element kernels have no profile
    # id, so the public API cannot show that pad_nhwc (and not some folded form) ran: the cases assert the convolution's id only and
    # check the padded VALUES -- the float64 model pads by reflection / replication, a zero-padded or unpadded input would not match
    _case("halo3_32_64_small", "c9s1-32,c3s1-64,c9s1-3", 1, (5, 20), [364], poison=True),
    _case("halo3_32_64_tile", "c9s1-32,c3s1-64,c9s1-3", 1, (8, 32), [364]),
    _case("halo3_32_64_ragged", "c9s1-32,c3s1-64,c9s1-3", 1, (17, 65), [364]),
    _case("halo3_32_64_wide_edge", "c9s1-32,c3s1-64,c9s1-3", 1, (9, 52), [364]),
    _case("halo3_32_128", "c9s1-32,c3s1-128,c9s1-3", 1, (9, 33), [428]),
    _case("halo3_two_stages_U2", "c9s1-32,U2,c3s1-64,c9s1-3", 2, (18, 66), [364]),
    _case("halo3_R64", "c9s1-64,R64,c9s1-3", 1, (9, 33), [364, 364]),
    _case("pad_reflect", "c9s1-32,c3s1-64,c9s1-3", 1, (9, 33), [364], padding_type="reflect"),
    _case("pad_replicate", "c9s1-32,c3s1-64,c9s1-3", 1, (9, 33), [364], padding_type="replicate"),
    _case("pad_reflect_U2", "c9s1-32,U2,c3s1-64,c9s1-3", 2, (18, 66), [364], padding_type="reflect"),
    # CK_FOLD: the last layer itself, 16-row x 128-column tiles; 128 / 256 input channels behind U2 only
    _case("fold_32_small", "c9s1-32,c9s1-3", 1, (9, 20), [1], poison=True),
    _case("fold_32_tile", "c9s1-32,c9s1-3", 1, (16, 128), [1]),
    _case("fold_32_ragged", "c9s1-32,c9s1-3", 1, (17, 129), [1]),
    _case("fold_64", "c9s1-64,c9s1-3", 1, (17, 40), [1]),
    _case("fold_32_U2", "c9s1-32,U2,c9s1-3", 2, (34, 66), [1]),
    _case("fold_128_U2", "c9s1-128,U2,c9s1-3", 2, (34, 66), [1]),
    _case("fold_256_U2", "c9s1-256,U2,c9s1-3", 2, (18, 34), [1]),
    # CK_TCONV (8 x 32 input-pixel tiles per phase): its operator test has no statistics variant
    _case("tconv_64_32", "c9s1-32,d64,u32,c9s1-3", 2, (18, 66), [832], poison=True),
    # the launched join of three blocks in a row (the pending form: DIAG_CASES)
    _case("join_launched", "c9s1-128,R128,R128,R128,c9s1-3", 3, (17, 17), [728, 728]),
]

# the kernels behind the diagnostic switches: one child process per set of switches (read once per process).  The same three sizes per
# kernel, and the smallest case of each once more in a second child behind NaN-poisoned LDS and memory
def _sizes(name, arch, index_of_L, ids, small, tile, ragged, **kw):
    return [_case(name + "_small", arch, index_of_L, small, ids, poison=True, **kw), _case(name + "_tile", arch, index_of_L, tile, ids, **kw),
            _case(name + "_ragged", arch, index_of_L, ragged, ids, **kw)]


DIAG_CASES = [
    ({"FAV_FIRST_1D": "1", "FAV_NO_S2W": "1"},
     _sizes("first1d", "c9s1-32,c9s1-3", 0, [6], (5, 40), (8, 64), (9, 65))                      # conv_first_tiles: 8 x 64
     + _sizes("s2halo", "c9s1-32,d64,c9s1-3", 1, [264], (3, 20), (4, 32), (5, 33))               # conv3s2_tiles: 4 x 32
     # conv_mblocks: 128 consecutive output pixels per block whatever the row length: 100 | 128 | 231 pixels
     + _sizes("generic_128", "c9s1-64,d128,c9s1-3", 1, [128], (5, 20), (4, 32), (7, 33))),
    ({"FAV_NO_S2W": "1", "FAV_NO_S2": "1", "FAV_NO_FIRST": "1", "FAV_NO_C8": "1"},
     _sizes("generic_64", "c9s1-32,d64,c9s1-3", 1, [64], (5, 20), (4, 32), (5, 33))
     + _sizes("generic_32", "c9s1-32,c9s1-3", 0, [32], (5, 20), (8, 16), (9, 33))),
    ({"FAV_NO_FIRST": "1", "FAV_WINO_F2": "1"},
     _sizes("c8d", "c9s1-32,c9s1-3", 0, [7], (5, 20), (8, 32), (9, 33))                          # conv_c8_tiles: 8 x 32
     + _sizes("wino_f2", "c9s1-128,R128,c9s1-3", 1, [528, 528], (5, 11), (8, 16), (17, 17))),    # conv3_wino_tiles: 8 x 16 units
    ({"FAV_NO_C8D": "1", "FAV_W4_GRID": "7", "FAV_LAZY_JOIN": "1"},
     _sizes("c8", "c9s1-32,c9s1-3", 0, [8], (5, 20), (8, 32), (9, 33))
     + [_case("wino4_stream_k", "c9s1-128,R128,c9s1-3", 1, (33, 33), [728, 728], poison=True),   # 9 units dealt to 7 shares: cut units
        # (a join stays pending between blocks of conv - InstanceNorm - ReLU - conv - InstanceNorm only: launched in the raw variant)
        _case("join_pending", "c9s1-128,R128,R128,R128,c9s1-3", 3, (17, 17), [729, 728], ids_raw=[728, 728])]),
]

def probe_for(case, variant, out_dir, regimes=False):
    import zlib
    kw = case["kw"]
    hw = tuple(input_size(case["arch"], case["L"], o, **kw) for o in case["out"])
    pr = probe_checkpoints(case["arch"], case["L"], variant, zlib.crc32(case["name"].encode()) % 100000, hw, out_dir, regimes=regimes,
                           bf16=case.get("bf16", False), **kw)
    pr.tol = TOL_RAW if (variant == "raw" or pr.direct) else TOL_STATS
    pr.conv0 = conv_index(case["arch"], case["L"])
    pr.ids = case["ids"] if variant == "stats" else case["ids_raw"]
    return pr


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_stats_edges.py
# every kernel family's statistics under the channel regimes: its ragged size of the tables above, and its one-tile size where a full
# tile is what matters (a full F(4x4) unit is where the accumulator words are largest)
def _named(name, poison=False):
    c = next(c for c in CASES + [c for _, cs in DIAG_CASES for c in cs] if c["name"] == name)
    return dict(c, poison=poison)


EDGE_CASES = [_named("wino4_R128_tile"), _named("wino4_R128_ragged", poison=True), _named("wino4_R256"), _named("first2d_7_32_ragged"),
              _named("s2w_32_64_ragged"), _named("s2w_64_128"), _named("up2_64_ragged"), _named("halo3_32_64_ragged", poison=True),
              _named("halo3_32_64_wide_edge"), _named("tconv_64_32"), _named("join_launched")]
EDGE_DIAG_CASES = [(env, [_named(c["name"]) for c in cs if not c["name"].endswith("_small") and (not c["name"].endswith("_tile") or c["name"] == "wino_f2_tile")])
                   for env, cs in DIAG_CASES]
# the F(4x4) accumulator cases once more in the partials form (in_finalize_kernel)
EDGE_PARTIALS_ENV = {"FAV_NO_ACC_STATS": "1"}
EDGE_PARTIALS_CASES = [_named(n) for n in ("wino4_R128_tile", "wino4_R128_ragged", "wino4_R256", "join_launched")]
# the element kernels that take statistics, L = U2 with its own InstanceNorm + ReLU (no convolution id to assert).  32 / 64 / 128 channels:
# stats_kernel<0|8|16>, res_add_stats_kernel<0|8|16>.  Physical sizes: 9 x 33 = 297 pixels (two full blocks of 128 and one of 41); the join
# 3 rows of 140 (two segments per row, 128 + 12)
ELEMENT_CASES = [_case("stats_u2_%d" % C, "c9s1-%d,U2,c9s1-3" % C, 1, (18, 66), []) for C in (32, 64, 128)] + \
                [_case("join_u2_%d" % C, "c9s1-%d,R%d,U2,c9s1-3" % (C, C), 2, (6, 280), []) for C in (32, 64, 128)]


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gpu_bf16_parity.py
# conv3_halo_bf16_kernel<BN, S2> (precision 1; ids as CK_HALO3: 364 for 64 filters, 428 for 128).  8 x 32 tiles only; sizes are L's output
def _bcase(name, arch, index_of_L, out, ids, poison=False, **kw):
    return dict(_case(name, arch, index_of_L, out, ids, poison=poison, **kw), bf16=True)


def bf16_units(case):
    """stream-K work units of L's (last) convolution: tiles of 8 x 32 times cin / 32 x 3 tap rows (launch_h3_t; an R<n> item is unpadded
    and keeps its channel count, so both of its convolutions have this many)"""
    items = case["arch"].split(",")
    v = items[case["L"] - 1]
    prev = items[case["L"] - 2] if v[0] == "U" else v
    cin = int(prev[5:]) if prev[0] == "c" else int(prev[1:])
    return -(-case["out"][0] // 8) * -(-case["out"][1] // 32) * (cin // 32) * 3


BF16_CASES = [
    # <64, false>: zero padding 1 (the mask path); under a tile | one tile | ragged | a 20-column right edge, which the fp32 kernel cuts
    # into 16 x 16 tiles and this one must not
    _bcase("bf16_64_small", "c9s1-32,c3s1-64,c9s1-3", 1, (5, 20), [364], poison=True),
    _bcase("bf16_64_tile", "c9s1-32,c3s1-64,c9s1-3", 1, (8, 32), [364]),
    _bcase("bf16_64_ragged", "c9s1-32,c3s1-64,c9s1-3", 1, (17, 65), [364]),
    _bcase("bf16_64_no_edge_tiles", "c9s1-32,c3s1-64,c9s1-3", 1, (9, 52), [364]),
    # <128, false>; R128: unpadded, both convolutions on the kernel, the second one behind a sparse first
    _bcase("bf16_128", "c9s1-32,c3s1-128,c9s1-3", 1, (9, 33), [428]),
    _bcase("bf16_R128_small", "c9s1-128,R128,c9s1-3", 1, (9, 11), [428, 428]),
    _bcase("bf16_R128_ragged", "c9s1-128,R128,c9s1-3", 1, (17, 33), [428, 428]),
    # <64, true>, <128, true>: two pending stages and ups = 1
    _bcase("bf16_64_U2", "c9s1-32,U2,c3s1-64,c9s1-3", 2, (18, 66), [364]),
    _bcase("bf16_128_U2", "c9s1-64,U2,c3s1-128,c9s1-3", 2, (18, 66), [428]),
    # behind the element kernel pad_nhwc
    _bcase("bf16_pad_reflect", "c9s1-32,c3s1-64,c9s1-3", 1, (9, 33), [364], padding_type="reflect"),
    _bcase("bf16_pad_replicate", "c9s1-32,c3s1-64,c9s1-3", 1, (9, 33), [364], padding_type="replicate"),
    # filter counts that run padded: the n < COUT store guard, zero channels in the statistics
    _bcase("bf16_48_as_64", "c9s1-32,c3s1-48,c9s1-3", 1, (9, 33), [364]),
    _bcase("bf16_96_as_128", "c9s1-32,c3s1-96,c9s1-3", 1, (9, 33), [428]),
]
# stream-K with cut tiles: 288 units = 12 tiles x 24 | 24 tiles x 12 -- at least 257 and no multiple of 256, so the grid is one block per
# CU on any MI355X and every tile's units are spread over several blocks, unit ranges starting mid-slice (tests/test_cpu_bf16_probe.py
# re-derives the counts)
BF16_SK_CASES = [
    _bcase("bf16_sk_256_128", "c9s1-256,c3s1-128,c9s1-3", 1, (17, 97), [428], poison=True),
    _bcase("bf16_sk_R128", "c9s1-128,R128,c9s1-3", 1, (41, 97), [428, 428], poison=True),
]
