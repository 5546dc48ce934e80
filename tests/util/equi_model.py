"""numpy restatement of fav_vr_equi_to_faces_rgb8 (csrc/kernels_equi.hip): one equirectangular frame -> six expanded cube faces.

Written from the formulas, not from the kernel.  Face k is processing position k = segment k of the strip fast_artistic_video_vr.lua:543
composes (segments 4 and 5 rotated by 180 degrees); the geometry is the inverse of fav_vr_map_host(kind 4, median_filter 0):

    (sx, sy) = (fx, fy) for k < 4, (wplus - 1 - fx, hplus - 1 - fy) for k >= 4
    a = (sx - overlap_w / 2) / (wplus - overlap_w) * 2 - 1,   b likewise along y
    (x, y, z) = k: 0 (a, b, 1)  1 (-1, b, a)  2 (1, b, -a)  3 (-a, b, -1)  4 (a, -1, b)  5 (a, 1, -b)
    phi = atan2(-x, -z) mod 2 pi,  theta = atan2(sqrt(x^2 + z^2), y),  u = phi W / (2 pi),  v = H (1 - theta / pi)

and the frame is sampled at (u, v) with the Catmull-Rom cubic (columns modulo W, rows clamped), along the row first.  An output pixel
is the mean of S x S samples at the sub-pixel centres (fx + (2 i + 1 - S) / (2 S), fy + (2 j + 1 - S) / (2 S)).

dtype=np.float64: the yardstick.  dtype=np.float32: the same steps with every operation rounded to fp32, in the kernel's order (its
constants 2 / (wplus - overlap), W / (2 pi), H / pi formed once) -- max|M32 - M64| is the fp32 error the GPU test's bound rests on.
"""
import numpy as np

PROC_ORDER = (6, 1, 2, 5, 3, 4)          # file id of processing position k (fast_artistic_video_vr.lua:103)


def catmull_rom(p0, p1, p2, p3, x):
    a1 = p2 - p0
    a2 = 2 * p0 - 5 * p1 + 4 * p2 - p3
    a3 = 3 * (p1 - p2) + p3 - p0
    return p1 + 0.5 * x * (a1 + x * (a2 + x * a3))


def direction(k, a, b):
    one = np.ones_like(a)
    return [(a, b, one), (-one, b, a), (one, b, -a), (-a, b, -one), (a, -one, b), (a, one, -b)][k]


def face_coordinates(k, px, py, hplus, wplus, overlap_w, overlap_h, ew, eh, dtype=np.float64):
    """(u, v) in the equirectangular frame of the face points (px, py) (arrays of `dtype`)"""
    f = dtype
    sx = px if k < 4 else f(wplus - 1) - px
    sy = py if k < 4 else f(hplus - 1) - py
    if f is np.float32:
        a = (sx - f(overlap_w) * f(0.5)) * (f(2) / f(wplus - overlap_w)) - f(1)
        b = (sy - f(overlap_h) * f(0.5)) * (f(2) / f(hplus - overlap_h)) - f(1)
    else:
        a = (sx - overlap_w / 2) / (wplus - overlap_w) * 2 - 1
        b = (sy - overlap_h / 2) / (hplus - overlap_h) * 2 - 1
    x, y, z = direction(k, a, b)
    phi = np.arctan2(-x, -z)
    phi = np.where(phi < 0, phi + f(2 * np.pi), phi)
    theta = np.arctan2(np.sqrt(x * x + z * z), y)
    if f is np.float32:
        return phi * f(ew / (2 * np.pi)), f(eh) - theta * f(eh / np.pi)
    return phi * ew / (2 * np.pi), eh * (1 - theta / np.pi)


def sample(equi, u, v, dtype=np.float64):
    """Catmull-Rom sample of equi (u8 [H][W][3]) at (u, v): [..., 3] of `dtype`"""
    eh, ew = equi.shape[:2]
    src = equi.astype(dtype)
    fu, fv = np.floor(u), np.floor(v)
    tx, ty = (u - fu)[..., None], (v - fv)[..., None]
    iu, iv = fu.astype(np.int64), fv.astype(np.int64)
    cols = [(iu - 1 + t) % ew for t in range(4)]
    rows = [np.clip(iv - 1 + r, 0, eh - 1) for r in range(4)]
    along = [catmull_rom(*[src[rows[r], cols[t]] for t in range(4)], tx) for r in range(4)]
    return catmull_rom(*along, ty)


def equi_to_faces(equi, hplus, wplus, overlap_w, overlap_h, supersample, dtype=np.float64):
    """-> (faces u8 [6][hplus][wplus][3], planes `dtype` [6][hplus][wplus][3] unrounded, 0..255 units)"""
    f, S = dtype, supersample
    eh, ew = equi.shape[:2]
    fy, fx = np.meshgrid(np.arange(hplus).astype(f), np.arange(wplus).astype(f), indexing="ij")
    planes = np.zeros((6, hplus, wplus, 3), f)
    for k in range(6):
        acc = np.zeros((hplus, wplus, 3), f)
        for j in range(S):
            py = fy + f(2 * j + 1 - S) / f(2 * S)
            for i in range(S):
                px = fx + f(2 * i + 1 - S) / f(2 * S)
                u, v = face_coordinates(k, px, py, hplus, wplus, overlap_w, overlap_h, ew, eh, f)
                acc = acc + sample(equi, u, v, f)
        planes[k] = acc / f(S * S)
    faces = np.clip(np.floor(planes + f(0.5)), 0, 255).astype(np.uint8)
    return faces, planes


# ---------------------------------------------------------------------------------------------- the way back (round-trip tests)
def strip(faces):
    """the strip of fast_artistic_video_vr.lua:543 / fav_vr_finish_frame: segments 0..3 as they are, 4 and 5 rotated by 180 degrees"""
    return np.concatenate([np.asarray(faces[k]) if k < 4 else np.asarray(faces[k])[::-1, ::-1] for k in range(6)], axis=1)


def sample_strip(strip_hwc, equi_map):
    """bilinear taps of the strip at (j + dy, i + dx), equi_map = fav_vr_map_host(kind 4): [2][out_h][out_w] -> float64 [out_h][out_w][3]"""
    s = strip_hwc.astype(np.float64)
    oh, ow = equi_map.shape[1:]
    jj, ii = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    yp, xp = jj + equi_map[0].astype(np.float64), ii + equi_map[1].astype(np.float64)
    y0, x0 = np.floor(yp).astype(np.int64), np.floor(xp).astype(np.int64)
    wy, wx = (yp - y0)[..., None], (xp - x0)[..., None]
    cy = lambda y: np.clip(y, 0, s.shape[0] - 1)
    cx = lambda x: np.clip(x, 0, s.shape[1] - 1)
    return ((1 - wy) * ((1 - wx) * s[cy(y0), cx(x0)] + wx * s[cy(y0), cx(x0 + 1)]) +
            wy * ((1 - wx) * s[cy(y0 + 1), cx(x0)] + wx * s[cy(y0 + 1), cx(x0 + 1)]))


# ---------------------------------------------------------------------------------------------- test images
def sphere_image(ew, eh, angle=0.0):
    """An equirectangular u8 image of a function of the DIRECTION (low-order polynomials of x, y, z per channel): no seam at longitude 0,
    every face and every orientation of a face distinguishable.  angle: the scene turned about the axis (1, 2, 3) / sqrt(14), radians."""
    j, i = np.meshgrid(np.arange(eh), np.arange(ew), indexing="ij")
    phi, theta = 2 * np.pi * i / ew, np.pi * (1 - j / eh)
    d = np.stack([-np.sin(phi) * np.sin(theta), np.cos(theta), -np.cos(phi) * np.sin(theta)], -1)
    if angle:
        n = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
        R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
        d = d @ R.T
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    rgb = np.stack([0.5 + 0.42 * x + 0.14 * y * z, 0.5 + 0.42 * y + 0.14 * x * z, 0.5 + 0.42 * z + 0.14 * x * y], -1)
    return np.clip(np.floor(rgb * 255 + 0.5), 0, 255).astype(np.uint8)


def write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


# ---------------------------------------------------------------------------------------------- the round trip and its gate
RT = dict(ew=192, eh=96, edge=48, overlap=8, supersample=2)      # the round-trip case of tests/test_cpu_equi.py
_rt = {}


def round_trip_error(faces, equi_map, source):
    """mean |sample(strip(faces), map) - source| in grey levels"""
    return float(np.abs(sample_strip(strip(faces), equi_map) - source).mean())


def round_trip_premise(vr_map_host):
    """-> dict(e_ok, e_bad, wrong={name: error}, gate, faces, planes, planes32, image, map): the fp64 model's faces taken back through the
    strip and fav_vr_map_host(kind 4) reproduce the source image (e_ok); each wrong variant of the transform does not (e_bad = the
    smallest of them); gate = sqrt(e_ok e_bad).  Computed once per process."""
    if _rt:
        return _rt
    c = RT
    img = sphere_image(c["ew"], c["eh"])
    faces, planes = equi_to_faces(img, c["edge"], c["edge"], c["overlap"], c["overlap"], c["supersample"], np.float64)
    _, planes32 = equi_to_faces(img, c["edge"], c["edge"], c["overlap"], c["overlap"], c["supersample"], np.float32)
    m = vr_map_host(4, c["edge"], c["edge"], c["overlap"], 0, c["ew"], c["eh"])
    wrong = {}
    swapped = list(faces); swapped[0], swapped[1] = faces[1], faces[0]
    wrong["faces 1 and 2 swapped"] = round_trip_error(swapped, m, img)
    unrot = list(faces); unrot[4] = faces[4][::-1, ::-1]
    wrong["face 5 not rotated"] = round_trip_error(unrot, m, img)
    mirrored = list(faces); mirrored[0] = faces[0][:, ::-1]
    wrong["face 1 mirrored"] = round_trip_error(mirrored, m, img)
    flat, _ = equi_to_faces(img, c["edge"], c["edge"], 0, 0, c["supersample"], np.float64)       # faces spanning +-1
    wrong["overlap margin ignored"] = round_trip_error(flat, m, img)
    e_ok, e_bad = round_trip_error(faces, m, img), min(wrong.values())
    _rt.update(e_ok=e_ok, e_bad=e_bad, wrong=wrong, gate=float(np.sqrt(e_ok * e_bad)), faces=faces, planes=planes, planes32=planes32,
               image=img, map=m)
    return _rt
