"""numpy model of the 360-degree post-processing (fav_vr_finish_frame behind the blend: csrc/kernels_vr.hip median3_kernel, median_kernel,
rotate_kernel / rot_src, strip_kernel, and the u8 quantisation), written independently of oracle/vr_oracle.py: index formulas from the
comments of kernels_vr.hip instead of transposes and reversals, a sort of a strided view instead of an unfolded copy.
tests/test_cpu_vr_post.py holds the two to each other; tests/test_gpu_vr_post.py holds the GPU to this one, bit for bit.

Also the face contents both tests use.  A plain face is coordinate-coded,
    face[c][y][x] = (k * 2^20 + y * 1024 + x) / 2^23 * 2^-c          (k: face 0..5, c: channel 0..2)
exact in fp32, in [0, 1), unique over the six faces of a channel, and a wrong channel decodes to another code: no wrong source pixel can
coincide with the right one.  Along a row and down a column the code increases, so the lower median of an r x r window is its centre.
numpy only."""
import numpy as np

F = np.float32
CUBE_ORDER = (3, 0, 4, 5, 2, 1)            # fast_artistic_video_vr.lua:542-552 (file ids 4, 1, 5, 6, 3, 2 as faces in processing order)
CUBE_ROT = (0, 0, 1, 2, 0, 0)              # 1 = rotate90, 2 = rotateMinus90
NAN_PER_FACE = 20


# ------------------------------------------------------------------------------------------------ operations
def median(img: np.ndarray, r: int) -> np.ndarray:
    """utils.lua:151-159: r x r windows, no padding, the (r*r-1)//2-th smallest (torch's lower median).  NaN sorts last."""
    if r <= 1:
        return np.ascontiguousarray(img, F)
    img = np.ascontiguousarray(img, F)
    win = np.lib.stride_tricks.sliding_window_view(img, (r, r), axis=(1, 2))
    c, hh, ww = win.shape[:3]
    return np.ascontiguousarray(np.sort(win.reshape(c, hh, ww, r * r), axis=-1)[..., (r * r - 1) // 2])


def nan_windows(img: np.ndarray, r: int) -> np.ndarray:
    """bool [C][H-r+1][W-r+1]: the windows that hold a NaN (what they return is unspecified)"""
    nan = np.isnan(np.ascontiguousarray(img, F))
    if r <= 1:
        return nan
    return np.lib.stride_tricks.sliding_window_view(nan, (r, r), axis=(1, 2)).any(axis=(-1, -2))


def rotate(t: np.ndarray, mode: int) -> np.ndarray:
    """kernels_vr.hip rot_src: src [C][H][W];
    1 rotate90      -> [C][W][H], dst[i][j] = src[j][W-1-i]
    2 rotateMinus90 -> [C][W][H], dst[i][j] = src[H-1-j][i]
    3 rotate180     -> [C][H][W], dst[i][j] = src[H-1-i][W-1-j]"""
    _, H, W = t.shape
    if mode == 0:
        return np.ascontiguousarray(t)
    dh, dw = (W, H) if mode in (1, 2) else (H, W)
    i, j = np.meshgrid(np.arange(dh), np.arange(dw), indexing="ij")
    if mode == 1:
        sy, sx = j, W - 1 - i
    elif mode == 2:
        sy, sx = H - 1 - j, i
    elif mode == 3:
        sy, sx = H - 1 - i, W - 1 - j
    else:
        raise ValueError(mode)
    return np.ascontiguousarray(t[:, sy, sx])


def equi_strip(filtered) -> np.ndarray:
    """the equirectangular warp's input (fast_artistic_video_vr.lua:538-541): faces 0..5 side by side, 4 and 5 rotated by 180 degrees"""
    c, fh, fw = filtered[0].shape
    out = np.empty((c, fh, 6 * fw), F)
    for k in range(6):
        out[:, :, k * fw:(k + 1) * fw] = rotate(filtered[k], 3 if k >= 4 else 0)
    return out


def cube_crop(hp: int, wp: int, overlap_w: int, overlap_h: int, med: int):
    """(ovh, ovw, ch, cw) of the cube-map strip in FILTERED-face coordinates (:515-516)"""
    r = med // 2
    ovh, ovw = overlap_h // 2 - r, overlap_w // 2 - r
    return ovh, ovw, hp - 2 * ovh, wp - 2 * ovw


def cube_strip(filtered, hp: int, wp: int, overlap_w: int, overlap_h: int, med: int) -> np.ndarray:
    """:542-552: crops of faces 3, 0, rot90(4), rotMinus90(5), 2, 1 side by side; square crops only"""
    ovh, ovw, ch, cw = cube_crop(hp, wp, overlap_w, overlap_h, med)
    if ch != cw:
        raise ValueError("the cube-map strip needs square cropped faces")
    c = filtered[0].shape[0]
    out = np.empty((c, ch, 6 * cw), F)
    for q in range(6):
        crop = filtered[CUBE_ORDER[q]][:, ovh:ovh + ch, ovw:ovw + cw]
        out[:, :, q * cw:(q + 1) * cw] = rotate(crop, CUBE_ROT[q])
    return out


def quantize(img: np.ndarray) -> np.ndarray:
    """planar f32 [3][H][W] -> u8 [H][W][3]: clip(x, 0, 1) * 255 truncated, all in fp32.  A NaN pixel (unspecified) is written as 0."""
    v = np.clip(np.nan_to_num(np.asarray(img, F), nan=0.0, posinf=np.inf, neginf=-np.inf), F(0), F(1)) * F(255)
    assert v.dtype == F
    return np.ascontiguousarray(np.transpose(v.astype(np.uint8), (1, 2, 0)))


# ------------------------------------------------------------------------------------------------ face contents
def _codes(n: int, k: int) -> np.ndarray:
    y, x = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    return k * (1 << 20) + y * 1024 + x


def _hash(code: np.ndarray, c: int) -> np.ndarray:
    h = (code.astype(np.uint64) * np.uint64(2654435761) + np.uint64(c) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF); h ^= h >> np.uint64(13)
    return h.astype(np.int64)


def coded_face(n: int, k: int) -> np.ndarray:
    assert 0 <= k < 6 and n <= 1024
    base = _codes(n, k).astype(np.float64) / float(1 << 23)
    out = np.stack([base * 2.0 ** -c for c in range(3)]).astype(F)
    assert np.array_equal(out.astype(np.float64), np.stack([base * 2.0 ** -c for c in range(3)]))      # exact in fp32
    return out


def decode(v: np.ndarray, c: int):
    """(face, y, x) of a coded value of channel c; -1 where it is no code"""
    code = np.asarray(v, np.float64) * float(1 << 23) * 2.0 ** c
    ok = np.isfinite(code) & (code == np.floor(code)) & (code >= 0) & (code < 6 * (1 << 20))
    ci = np.where(ok, code, -1).astype(np.int64)
    return np.where(ok, ci >> 20, -1), np.where(ok, (ci >> 10) & 1023, -1), np.where(ok, ci & 1023, -1)


def nan_positions(n: int, k: int):
    """20 fixed positions per face, at least 12 pixels apart and more than a quarter of the face away from every edge: no blend
    warp samples them, so each stays one NaN of its own face"""
    ys = n // 4 + 3 * k + (n // 2 // 5) * np.arange(5)
    xs = n // 4 + 2 * k + (n // 2 // 4) * np.arange(4)
    return [(int(y), int(x)) for y in ys for x in xs]


SPECIALS = [-0.0, 0.0, 1.0, 254.999 / 255, 255.001 / 255, 1 / 255, 0.999 / 255, -1e-30, 1 + 1e-7, 1e-40, 2.0, -5.0, 0.5, 127.5 / 255,
            128 / 255, 254 / 255]


def faces(n: int, variant: str = "coded"):
    """six faces [3][n][n] f32.  variant: coded | ties (8 levels, every window has ties) | inf (coded, about 2 % +-inf in the middle half
    of the face, single ones and clusters) | range (multiples of 1/255 and their fp32 neighbours from -0.5 to 1.5, and SPECIALS, for the
    quantiser) | nan (coded with NAN_PER_FACE isolated NaNs)"""
    out = []
    q0, q1 = n // 4, n - n // 4
    for k in range(6):
        code = _codes(n, k)
        f = coded_face(n, k)
        if variant == "ties":
            f = np.stack([(_hash(code, c) % 8).astype(F) / F(8) for c in range(3)])
        elif variant == "inf":
            for c in range(3):
                h = _hash(code >> 1, c) % 50                      # (pairs of columns share a hash: clusters of two, and more by chance)
                mid = np.zeros((n, n), bool); mid[q0:q1, q0:q1] = True
                f[c][mid & (h == 0)] = np.inf
                f[c][mid & (h == 1)] = -np.inf
        elif variant == "range":
            for c in range(3):
                h = _hash(code, c)
                j = (h % 511 - 127).astype(F) / F(255)             # -127/255 .. 383/255
                step = (h >> 10) % 3
                f[c] = np.where(step == 0, j, np.where(step == 1, np.nextafter(j, F(np.inf)), np.nextafter(j, F(-np.inf)))).astype(F)
                f[c, n // 2, q0:q0 + len(SPECIALS)] = np.array(SPECIALS, F)
        elif variant == "nan":
            for (y, x) in nan_positions(n, k):
                f[:, y, x] = np.nan
        elif variant != "coded":
            raise ValueError(variant)
        out.append(np.ascontiguousarray(f, F))
    return out


def cube_sources(hp: int, overlap_w: int, overlap_h: int, med: int):
    """Model-free statement of the cube-map strip for coded square faces, from the definition alone: (face, y, x, interior), each
    [ch][6 cw], of the RAW face pixel every strip pixel shows -- segment q holds face CUBE_ORDER[q], cropped from overlap/2 on in face
    coordinates (the median of a coded window is its centre, so the filter's r // 2 shift and the crop's `- r` cancel), rotated by
    CUBE_ROT[q].  interior: the median window of that pixel lies where the blend leaves the face untouched (gradient masks are 0 more
    than overlap - 10 pixels from an edge), so the strip must hold that pixel's code exactly."""
    r = med // 2
    oy, ox = overlap_h // 2, overlap_w // 2
    ch, cw = hp - 2 * (oy - r), hp - 2 * (ox - r)          # the crop {ov + 1, hplus - ov} is taken with the UNFILTERED hplus (:548): 2 r larger
    assert ch == cw
    i, j = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
    face = np.empty((ch, 6 * cw), np.int64); yy = np.empty_like(face); xx = np.empty_like(face)
    for q in range(6):
        if CUBE_ROT[q] == 0:
            cy, cx = i, j
        elif CUBE_ROT[q] == 1:                     # rotate90: dst[i][j] = src[j][W-1-i]
            cy, cx = j, cw - 1 - i
        else:                                      # rotateMinus90: dst[i][j] = src[H-1-j][i]
            cy, cx = ch - 1 - j, i
        face[:, q * cw:(q + 1) * cw] = CUBE_ORDER[q]; yy[:, q * cw:(q + 1) * cw] = cy + oy; xx[:, q * cw:(q + 1) * cw] = cx + ox
    gh, gw = overlap_h - 10, overlap_w - 10
    interior = (yy - r >= gh) & (yy + r < hp - gh) & (xx - r >= gw) & (xx + r < hp - gw)
    return face, yy, xx, interior
