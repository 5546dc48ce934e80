"""numpy restatement of csrc/kernels_yuv.hip ("Y4M in and out"): 8-bit YCbCr planes <-> RGB bytes, 4:4:4 and 4:2:0 with
centre (C420jpeg) or left (C420mpeg2) chroma siting, BT.601 / BT.709, limited / full range.  Every operation is written in the order the
kernels perform it; with dtype=np.float32 each one rounds like theirs (the unit is compiled without FMA contraction), so the kernels are
held to this model byte for byte.  dtype=np.float64 is the same arithmetic with unrounded constants: the yardstick of the fp32 model.
Also the few lines of YUV4MPEG2 container the tests need."""
from collections import namedtuple

import numpy as np

Format = namedtuple("Format", "chroma siting matrix full_range", defaults=("420", "center", "601", False))
KR_KB = {"601": (0.299, 0.114), "709": (0.2126, 0.0722)}
ALL_FORMATS = [Format(c, s, m, r) for c, s in (("420", "center"), ("420", "left"), ("444", "center"))
               for m in ("601", "709") for r in (False, True)]


def constants(fmt, dtype=np.float32):
    """every constant in double, rounded once to dtype"""
    kr, kb = KR_KB[fmt.matrix]
    kg = 1.0 - kr - kb
    sy, sc, oy = (1.0, 1.0, 0.0) if fmt.full_range else (219.0 / 255.0, 224.0 / 255.0, 16.0)
    k_r = 2.0 * (1.0 - kr) / sc
    k_b = 2.0 * (1.0 - kb) / sc
    c = dict(kr=kr, kg=kg, kb=kb, sy=sy, oy=oy, cbs=sc / (2.0 * (1.0 - kb)), crs=sc / (2.0 * (1.0 - kr)),
             isy=1.0 / sy, kR=k_r, kB=k_b, kGr=k_r * kr / kg, kGb=k_b * kb / kg)
    return {k: dtype(v) for k, v in c.items()}


def chroma_shape(W, H, fmt):
    return (H, W) if fmt.chroma == "444" else ((H + 1) // 2, (W + 1) // 2)


def frame_bytes(W, H, fmt):
    hc, wc = chroma_shape(W, H, fmt)
    return W * H + 2 * hc * wc


def split_planes(yuv, W, H, fmt):
    hc, wc = chroma_shape(W, H, fmt)
    yuv = np.asarray(yuv, np.uint8).reshape(-1)
    assert yuv.size == frame_bytes(W, H, fmt)
    return yuv[:W * H].reshape(H, W), yuv[W * H:W * H + hc * wc].reshape(hc, wc), yuv[W * H + hc * wc:].reshape(hc, wc)


def quantise(x):
    """floor(x + 0.5) clamped to [0, 255]"""
    return np.clip(np.floor(x + x.dtype.type(0.5)), 0, 255).astype(np.uint8)


def quantise_f32_image(rgb_planar):
    """image.save's rule (fav_png_encode_f32): clamp to [0, 1], x255, truncate; planar [3][H][W] -> bytes [H][W][3]"""
    v = np.clip(np.asarray(rgb_planar, np.float32), np.float32(0), np.float32(1)) * np.float32(255)
    return np.ascontiguousarray(np.transpose(v.astype(np.uint8), (1, 2, 0)))


# ---------------------------------------------------------------------------------------------- RGB -> YCbCr
def rgb_to_ycbcr_unquantised(rgb_hwc, fmt, dtype=np.float32):
    """(Y, Cb, Cr) of every pixel before quantisation, [H][W] each"""
    k = constants(fmt, dtype)
    R, G, B = (np.asarray(rgb_hwc)[..., c].astype(dtype) for c in range(3))
    y = (k["kr"] * R + k["kg"] * G) + k["kb"] * B
    Y = y * k["sy"] + k["oy"]
    Cb = (B - y) * k["cbs"] + dtype(128)
    Cr = (R - y) * k["crs"] + dtype(128)
    return Y, Cb, Cr


def _pad_to(c, h2, w2):
    """replicated edge up to h2 x w2"""
    return np.pad(c, ((0, h2 - c.shape[0]), (0, w2 - c.shape[1])), mode="edge")


def downsample_chroma(c, siting):
    """unquantised chroma [H][W] -> [ceil(H/2)][ceil(W/2)]; a missing partner is the replicated edge sample"""
    dt = c.dtype.type
    H, W = c.shape
    hc, wc = (H + 1) // 2, (W + 1) // 2
    if siting == "center":
        p = _pad_to(c, 2 * hc, 2 * wc)
        return ((p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2])) * dt(0.25)
    xs = 2 * np.arange(wc)
    left, right = c[:, np.clip(xs - 1, 0, W - 1)], c[:, np.clip(xs + 1, 0, W - 1)]
    cen = c[:, xs]
    h = ((left + right) + (cen + cen)) * dt(0.25)
    h = _pad_to(h, 2 * hc, wc)
    return (h[0::2] + h[1::2]) * dt(0.5)


def rgb_to_yuv(rgb_hwc, fmt, dtype=np.float32):
    """bytes [H][W][3] -> the frame's payload: Y, Cb, Cr planes, flat uint8"""
    Y, Cb, Cr = rgb_to_ycbcr_unquantised(rgb_hwc, fmt, dtype)
    if fmt.chroma == "420":
        Cb, Cr = downsample_chroma(Cb, fmt.siting), downsample_chroma(Cr, fmt.siting)
    return np.concatenate([quantise(p).reshape(-1) for p in (Y, Cb, Cr)])


def rgb_f32_to_yuv(rgb_planar, fmt, dtype=np.float32):
    """planar fp32 [3][H][W] -> payload: the conversion of exactly the bytes the PNG would have held"""
    return rgb_to_yuv(quantise_f32_image(rgb_planar), fmt, dtype)


# ---------------------------------------------------------------------------------------------- YCbCr -> RGB
def _up_centre(c, n, axis):
    """row 2j: 0.25 C[j-1] + 0.75 C[j]; row 2j+1: 0.75 C[j] + 0.25 C[j+1]; indices clamped; n output samples"""
    dt = c.dtype.type
    m = c.shape[axis]
    x = np.arange(n)
    j = x // 2
    other = np.clip(np.where(x % 2 == 0, j - 1, j + 1), 0, m - 1)
    a, b = np.take(c, other, axis), np.take(c, j, axis)
    return dt(0.25) * a + dt(0.75) * b


def _up_left(c, n, axis):
    """column 2j: C[j]; column 2j+1: 0.5 (C[j] + C[j+1]); indices clamped"""
    dt = c.dtype.type
    m = c.shape[axis]
    x = np.arange(n)
    j = x // 2
    a, b = np.take(c, j, axis), np.take(c, np.clip(j + 1, 0, m - 1), axis)
    odd = (x % 2 == 1).reshape([-1 if d == axis else 1 for d in range(c.ndim)])
    return np.where(odd, dt(0.5) * (a + b), a)


def upsample_chroma(c, W, H, siting, dtype=np.float32):
    """a 4:2:0 chroma plane interpolated bilinearly to the W x H luma grid (before the matrix)"""
    c = np.asarray(c).astype(dtype)
    v = _up_centre(c, H, 0)
    return _up_centre(v, W, 1) if siting == "center" else _up_left(v, W, 1)


def yuv_to_rgb(yuv, W, H, fmt, dtype=np.float32):
    """payload -> bytes [H][W][3]"""
    k = constants(fmt, dtype)
    Yp, Cbp, Crp = split_planes(yuv, W, H, fmt)
    if fmt.chroma == "420":
        Cb, Cr = upsample_chroma(Cbp, W, H, fmt.siting, dtype), upsample_chroma(Crp, W, H, fmt.siting, dtype)
    else:
        Cb, Cr = Cbp.astype(dtype), Crp.astype(dtype)
    y = (Yp.astype(dtype) - k["oy"]) * k["isy"]
    cb, cr = Cb - dtype(128), Cr - dtype(128)
    R = y + k["kR"] * cr
    B = y + k["kB"] * cb
    G = (y - k["kGr"] * cr) - k["kGb"] * cb
    return np.stack([quantise(R), quantise(G), quantise(B)], axis=-1)


# ---------------------------------------------------------------------------------------------- YUV4MPEG2
C_TAG = {("420", "center"): "C420jpeg", ("420", "left"): "C420mpeg2", ("444", "center"): "C444", ("444", "left"): "C444"}


def y4m_header(W, H, fmt, extra="F25:1 Ip A1:1"):
    tags = [f"W{W}", f"H{H}"] + extra.split() + [C_TAG[(fmt.chroma, fmt.siting)]]
    if fmt.full_range:
        tags.append("XCOLORRANGE=FULL")
    return "YUV4MPEG2 " + " ".join(tags) + "\n"


def write_y4m(path, header, frames):
    with open(path, "wb") as f:
        f.write(header.encode())
        for fr in frames:
            f.write(b"FRAME\n")
            f.write(np.asarray(fr, np.uint8).tobytes())


def parse_y4m(data, frame_size):
    """bytes of a stream -> (header line without the newline, list of payloads); frame_size(W, H) gives a payload's length"""
    nl = data.index(b"\n")
    header = data[:nl].decode()
    tags = header.split(" ")
    assert tags[0] == "YUV4MPEG2", header
    W = int(next(t for t in tags[1:] if t[0] == "W")[1:])
    H = int(next(t for t in tags[1:] if t[0] == "H")[1:])
    n = frame_size(W, H)
    pos, frames = nl + 1, []
    while pos < len(data):
        e = data.index(b"\n", pos)
        assert data[pos:pos + 5] == b"FRAME", data[pos:pos + 16]
        assert e + 1 + n <= len(data), "truncated frame"
        frames.append(np.frombuffer(data[e + 1:e + 1 + n], np.uint8))
        pos = e + 1 + n
    return header, frames
