"""The `f<k>s<s>-<n>` (nn.SpatialFullConvolution, pad (k - 1) / 2, adj s - 1) and `C<n>` (non-residual conv block) items of the reference's
architecture grammar (models_video.lua:10-39,81-89,103-108): the emitter builds them as the reference does for every padding_type, both
.t7 readers agree on them, and the oracle's forward matches a PyTorch fp64 restatement of the same module list.  No GPU."""
import numpy as np
import pytest

from fav_amd import t7

ARCH = "c9s1-8,d16,C16,R16,f5s2-8,f3s1-8,c9s1-3"
H, W = 24, 20


def _torch_forward(layers, x):
    """the layer list in torch, double precision [recalled semantics of Torch7's modules, SURVEY.md Appendix C]"""
    import torch
    import torch.nn.functional as F
    T = lambda a: torch.from_numpy(np.asarray(a)).double()
    for L in layers:
        t = L["type"]
        if t == "pad": x = F.pad(x, (L["l"], L["r"], L["t"], L["b"]), mode="replicate" if L["mode"] == "replicate" else "reflect")
        elif t == "conv": x = F.conv2d(x, T(L["w"]), None if L["b"] is None else T(L["b"]), L["stride"], L["pad"])
        elif t == "fullconv": x = F.conv_transpose2d(x, T(L["w"]), None if L["b"] is None else T(L["b"]), stride=L["stride"], padding=L["pad"], output_padding=L["adj"])
        elif t == "in": x = F.instance_norm(x, weight=T(L["gamma"]), bias=T(L["beta"]), eps=L["eps"])
        elif t == "bn": x = F.batch_norm(x, T(L["mean"]), T(L["var"]), T(L["gamma"]), T(L["beta"]), False, 0.1, L["eps"])
        elif t == "relu": x = F.relu(x)
        elif t == "up": x = F.interpolate(x, scale_factor=L["s"], mode="nearest")
        elif t == "res":
            y = _torch_forward(L["block"], x); s = L["shave"]
            x = y + (x[:, :, s:-s, s:-s] if s else x)
        elif t == "tanh": x = torch.tanh(x)
        elif t == "mul": x = x * L["k"]
        elif t == "identity": pass
        else: raise ValueError(t)
    return x


@pytest.mark.parametrize("ptype", t7.PADDING_TYPES)
def test_f_and_C_items_every_padding_type(oracle, favlib, tmp_path, ptype):
    import torch
    p = str(tmp_path / "m.t7")
    t7.make_synthetic_checkpoint(p, arch=ARCH, seed=3, padding_type=ptype)
    model = t7.load(p)["model"]
    layers = t7.extract_layers(model)
    # the C block is a NESTED nn.Sequential (models_video.lua:106), followed by a ReLU and no further norm (:107-108)
    top = [m.cls for m in t7._seq(model["modules"])]
    assert top.count("nn.Sequential") == 2 and top.count("nn.SpatialFullConvolution") == 2
    mods = t7._seq(model["modules"])
    ic = next(i for i, m in enumerate(mods) if m.cls == "nn.Sequential" and t7._seq(m["modules"])[0].cls != "nn.ConcatTable")
    inner = [m.cls for m in t7._seq(mods[ic]["modules"])]
    padcls = {"reflect": "nn.SpatialReflectionPadding", "replicate": "nn.SpatialReplicationPadding"}.get(ptype)
    want = ["nn.SpatialConvolution", "nn.InstanceNormalization", "nn.ReLU", "nn.SpatialConvolution", "nn.InstanceNormalization"]
    if padcls: want = [padcls] + want[:3] + [padcls] + want[3:]
    assert inner == want and mods[ic + 1].cls == "nn.ReLU"
    convs = [m for m in t7._seq(mods[ic]["modules"]) if m.cls == "nn.SpatialConvolution"]
    assert all(int(c["padW"]) == (1 if ptype == "zero" else 0) and int(c["kW"]) == 3 and int(c["dW"]) == 1 for c in convs)
    # the lazily inserted front pad: the C block counts like the R block (2 px per side each at 1/2 resolution)
    if ptype == "reflect-start": assert layers[0]["type"] == "pad" and layers[0]["l"] == 8
    # both readers agree; the product's reader lists the transposed layers with their (k, s, p, adj) -- the stride-1 one as it is in the file
    text = favlib.describe_t7(p)
    assert text == favlib.describe_layers(layers)
    assert "fullconv 16 8 5 2 2 adj=1 bias=1\n" in text and "fullconv 8 8 3 1 1 adj=0 bias=1\n" in text
    full = [L for L in layers if L["type"] == "fullconv"]
    assert [(L["w"].shape, L["stride"], L["pad"], L["adj"]) for L in full] == [((16, 8, 5, 5), 2, 2, 1), ((8, 8, 3, 3), 1, 1, 0)]
    # oracle vs the torch restatement
    x = np.random.default_rng(2).standard_normal((7, H, W)).astype(np.float32)
    y = oracle.net_forward(layers, x)
    ref = _torch_forward(layers, torch.from_numpy(x)[None].double())[0].numpy()
    assert y.shape == ref.shape and (ptype == "none" or y.shape == (3, H, W))
    assert np.abs(y - ref).max() < 2e-3, float(np.abs(y - ref).max())      # (the tolerance of test_cpu_oracle.py for tiny_net_io)


def test_batchnorm_blocks_and_a_stride3_pair(oracle, favlib, tmp_path):
    """use_instance_norm = 0 puts SpatialBatchNormalization inside the C block too; c3s3 / f3s3 close on multiples of 3"""
    import torch
    p = str(tmp_path / "m.t7")
    t7.make_synthetic_checkpoint(p, arch="c9s1-8,c3s3-16,C16,f3s3-8,c9s1-3", seed=4, padding_type="zero", use_instance_norm=False, in_channels=3)
    layers = t7.extract_layers(t7.load(p)["model"])
    text = favlib.describe_t7(p)
    assert text == favlib.describe_layers(layers) and "fullconv 16 8 3 3 1 adj=2 bias=1\n" in text
    assert [L["type"] for L in layers].count("bn") == 5 and not any(L["type"] == "in" for L in layers)
    x = np.random.default_rng(5).standard_normal((3, H, 21)).astype(np.float32)
    y = oracle.net_forward(layers, x)
    ref = _torch_forward(layers, torch.from_numpy(x)[None].double())[0].numpy()
    assert y.shape == ref.shape == (3, H, 21) and np.abs(y - ref).max() < 2e-3


def test_even_filter_size_is_refused_with_a_message():
    with pytest.raises(ValueError, match="odd filter size"):
        t7.build_model("c9s1-8,d16,f4s2-8,c9s1-3")
