"""numpy restatement of csrc/kernels_yuv_layout.hip (include/fav_yuv.h; DESIGN.md, "Y4M in and out"): YCbCr planes of every layout --
4:2:0, 4:2:2, 4:4:4 at 8, 9, 10, 12, 14 or 16 bits per sample -- <-> RGB bytes.  It is yuv_model.py's arithmetic with the depth in the
constants, in the kernels' order of operations: with dtype=np.float32 every operation rounds like theirs (no FMA contraction), so the
kernels are held to it sample for sample; dtype=np.float64 is the same arithmetic with unrounded constants, the fp32 model's yardstick.
Samples are numpy integers (uint8 at depth 8, else uint16); payload() / samples_of() move between them and a frame's bytes."""
from collections import namedtuple

import numpy as np

import yuv_model as M

Layout = namedtuple("Layout", "chroma siting matrix full_range depth", defaults=("420", "center", "601", False, 8))
DEPTHS = (8, 9, 10, 12, 14, 16)
SAMPLINGS = (("420", "center"), ("420", "left"), ("422", "center"), ("422", "left"), ("444", "center"))


def constants(lay, dtype=np.float32):
    """m = 2^(D-8), q = (2^D - 1)/255; every constant in double, rounded once to dtype"""
    kr, kb = M.KR_KB[lay.matrix]
    kg = 1.0 - kr - kb
    D = lay.depth
    m, q = float(1 << (D - 8)), float((1 << D) - 1) / 255.0
    sy, sc, oy = (q, q, 0.0) if lay.full_range else (219.0 / 255.0 * m, 224.0 / 255.0 * m, 16.0 * m)
    k_r = 2.0 * (1.0 - kr) / sc
    k_b = 2.0 * (1.0 - kb) / sc
    c = dict(kr=kr, kg=kg, kb=kb, sy=sy, oy=oy, cbs=sc / (2.0 * (1.0 - kb)), crs=sc / (2.0 * (1.0 - kr)),
             isy=1.0 / sy, kR=k_r, kB=k_b, kGr=k_r * kr / kg, kGb=k_b * kb / kg, oc=float(1 << (D - 1)), qmax=float((1 << D) - 1))
    return {k: dtype(v) for k, v in c.items()}


def sample_dtype(lay):
    return np.uint8 if lay.depth == 8 else np.dtype("<u2")


def chroma_shape(W, H, lay):
    return {"444": (H, W), "422": (H, (W + 1) // 2), "420": ((H + 1) // 2, (W + 1) // 2)}[lay.chroma]


def frame_samples(W, H, lay):
    hc, wc = chroma_shape(W, H, lay)
    return W * H + 2 * hc * wc


def frame_bytes(W, H, lay):
    return frame_samples(W, H, lay) * (1 if lay.depth == 8 else 2)


def payload(samples, lay):
    """flat samples -> the frame's bytes (uint8 array): two bytes per sample, little-endian, above depth 8"""
    return np.ascontiguousarray(np.asarray(samples).astype(sample_dtype(lay))).view(np.uint8).reshape(-1)


def samples_of(data, lay):
    """a frame's bytes -> flat samples"""
    return np.frombuffer(np.ascontiguousarray(np.asarray(data, np.uint8)).tobytes(), sample_dtype(lay))


def split_planes(samples, W, H, lay):
    hc, wc = chroma_shape(W, H, lay)
    s = np.asarray(samples).reshape(-1)
    assert s.size == frame_samples(W, H, lay)
    return s[:W * H].reshape(H, W), s[W * H:W * H + hc * wc].reshape(hc, wc), s[W * H + hc * wc:].reshape(hc, wc)


def quantise(x, qmax):
    """floor(x + 0.5) clamped to [0, qmax]"""
    return np.clip(np.floor(x + x.dtype.type(0.5)), 0, qmax).astype(np.uint16 if qmax > 255 else np.uint8)


# ---------------------------------------------------------------------------------------------- RGB -> YCbCr
def ycbcr_unquantised(R, G, B, lay, dtype=np.float32):
    """R, G, B: [H][W] of dtype on the 0 .. 255 scale (bytes, or unquantised floats)"""
    k = constants(lay, dtype)
    y = (k["kr"] * R + k["kg"] * G) + k["kb"] * B
    Y = y * k["sy"] + k["oy"]
    Cb = (B - y) * k["cbs"] + k["oc"]
    Cr = (R - y) * k["crs"] + k["oc"]
    return Y, Cb, Cr


def downsample_422(c, siting):
    """unquantised chroma [H][W] -> [H][ceil(W/2)]: the horizontal rule of each siting alone; a missing partner is the edge sample"""
    dt = c.dtype.type
    H, W = c.shape
    wc = (W + 1) // 2
    xs = 2 * np.arange(wc)
    right = c[:, np.clip(xs + 1, 0, W - 1)]
    cen = c[:, xs]
    if siting == "center":
        return (cen + right) * dt(0.5)
    left = c[:, np.clip(xs - 1, 0, W - 1)]
    return ((left + right) + (cen + cen)) * dt(0.25)


def _encode(R, G, B, lay, dtype):
    Y, Cb, Cr = ycbcr_unquantised(R, G, B, lay, dtype)
    if lay.chroma == "420":
        Cb, Cr = M.downsample_chroma(Cb, lay.siting), M.downsample_chroma(Cr, lay.siting)
    elif lay.chroma == "422":
        Cb, Cr = downsample_422(Cb, lay.siting), downsample_422(Cr, lay.siting)
    qmax = (1 << lay.depth) - 1
    return np.concatenate([quantise(p, qmax).reshape(-1) for p in (Y, Cb, Cr)]).astype(sample_dtype(lay))


def rgb_to_yuv(rgb_hwc, lay, dtype=np.float32):
    """bytes [H][W][3] -> the frame's samples, flat"""
    R, G, B = (np.asarray(rgb_hwc)[..., c].astype(dtype) for c in range(3))
    return _encode(R, G, B, lay, dtype)


def rgb_f32_to_yuv(rgb_planar, lay, dtype=np.float32):
    """planar fp32 [3][H][W] -> samples.  Depth 8: image.save's truncation in front (yuv_model.quantise_f32_image); deeper: the floats
    enter unquantised, R = clamp(x, 0, 1) * 255 (formed in fp32 in both models: it is the input)"""
    if lay.depth == 8:
        return rgb_to_yuv(M.quantise_f32_image(rgb_planar), lay, dtype)
    v = np.clip(np.asarray(rgb_planar, np.float32), np.float32(0), np.float32(1)) * np.float32(255)
    return _encode(v[0].astype(dtype), v[1].astype(dtype), v[2].astype(dtype), lay, dtype)


# ---------------------------------------------------------------------------------------------- YCbCr -> RGB
def upsample_422(c, W, siting, dtype=np.float32):
    c = np.asarray(c).astype(dtype)
    return M._up_centre(c, W, 1) if siting == "center" else M._up_left(c, W, 1)


def yuv_to_rgb(samples, W, H, lay, dtype=np.float32):
    """samples (each taken as the number it is, no masking) -> bytes [H][W][3]"""
    k = constants(lay, dtype)
    Yp, Cbp, Crp = split_planes(samples, W, H, lay)
    if lay.chroma == "420":
        Cb, Cr = M.upsample_chroma(Cbp, W, H, lay.siting, dtype), M.upsample_chroma(Crp, W, H, lay.siting, dtype)
    elif lay.chroma == "422":
        Cb, Cr = upsample_422(Cbp, W, lay.siting, dtype), upsample_422(Crp, W, lay.siting, dtype)
    else:
        Cb, Cr = Cbp.astype(dtype), Crp.astype(dtype)
    y = (Yp.astype(dtype) - k["oy"]) * k["isy"]
    cb, cr = Cb - k["oc"], Cr - k["oc"]
    R = y + k["kR"] * cr
    B = y + k["kB"] * cb
    G = (y - k["kGr"] * cr) - k["kGb"] * cb
    return np.stack([M.quantise(R), M.quantise(G), M.quantise(B)], axis=-1)


# ---------------------------------------------------------------------------------------------- YUV4MPEG2
def c_tag(lay):
    """the header's C tag; None where the grammar has none (4:2:2 centre-sited, left-sited 4:2:0 above 8 bits)"""
    if lay.chroma == "444":
        base = "444"
    elif lay.chroma == "422":
        if lay.siting != "left":
            return None
        base = "422"
    elif lay.depth == 8:
        return "C420mpeg2" if lay.siting == "left" else "C420jpeg"
    else:
        if lay.siting == "left":
            return None
        base = "420"
    return "C" + base + ("" if lay.depth == 8 else f"p{lay.depth}")
