"""numpy model of what a cube face's network reads (csrc/vr.cpp vr_face, csrc/kernels_vr.hip): the border sum of the neighbours' faces, the
prior, and the eight floats per pixel of the reflection-padded input -- tests/test_cpu_vr_input.py, tests/test_gpu_vr_input.py.

Written from the reference's lines, fp32, one rounding per operation, and from nothing of the library:
  fast_artistic_video_vr.lua:130-144   the rotations (as index copies)
  fast_artistic_video_vr.lua:170-189   the static masks (warps of ones) and gradient masks, utils.lua:179-213
  fast_artistic_video_vr.lua:248-272   the border sum: one (source face, rotation, map) per term, TABLE below
  fast_artistic_video_vr.lua:275-294   the prior
  fast_artistic_video_core.lua:108-117, 161-171 and preprocess.lua:48, 57-62   the input assembly
It does not call oracle/vr_oracle.py's VRStylizer (_prior, _cert, _fill): tests/test_cpu_vr_input.py compares the two restatements.
The warp is a parameter (warp_fn(img [C][H][W], map [2][H][W]) -> [C][H][W]): vr_oracle.warp on the CPU, the library's own warp
operator on the GPU.  The uniform-random fill is vr_oracle.fill_uniform, the documented stand-in for the reference's unseeded torch.rand."""
import numpy as np

F = np.float32
MEAN = np.array([103.939, 116.779, 123.68], F)          # BGR (preprocess.lua:48)
L, R, T, B = "left", "right", "top", "bottom"
ROT0, ROT90, ROTM90, ROT180 = 0, 1, 2, 3

# fast_artistic_video_vr.lua:248-272 with last_segments[k + 1] = face k: the terms of face `mode`'s border sum in the reference's order,
# (source face, rotation, map); modes 4 and 5 divide every term by mask_all_div before it is added
TABLE = {
    0: (),
    1: ((0, ROT0, L),),                                                              # :250
    2: ((0, ROT0, R),),                                                              # :253
    3: ((1, ROT0, L), (2, ROT0, R)),                                                 # :256-257
    4: ((1, ROT90, L), (2, ROTM90, R), (3, ROT0, T), (0, ROT180, B)),                # :260-263
    5: ((1, ROTM90, L), (2, ROT90, R), (0, ROT180, T), (3, ROT0, B)),                # :266-269
}
DIVIDED = (4, 5)


def rotate(t, rot):
    """:130-144 on [C][H][W] as index copies.  rotate90 = reverse(transpose(2, 3), 2): out[i][j] = t[j][W - 1 - i];
    rotateMinus90 = reverse(transpose(2, 3), 3): out[i][j] = t[H - 1 - j][i]; rotate180: out[i][j] = t[H - 1 - i][W - 1 - j]"""
    _, h, w = t.shape
    if rot == ROT0:
        return t
    if rot == ROT180:
        i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        return np.ascontiguousarray(t[:, h - 1 - i, w - 1 - j])
    i, j = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")          # the result is [C][W][H]
    return np.ascontiguousarray(t[:, j, w - 1 - i] if rot == ROT90 else t[:, h - 1 - j, i])


def static_masks(warp_fn, maps):
    """:170-179: {left, right, top, bottom: warp(ones, map) [H][W]; all_div = max(l + r + t + b, 1); all = min(.., 1)}"""
    h, w = maps[L].shape[1:]
    ones = np.ones((1, h, w), F)
    m = {k: np.asarray(warp_fn(ones, maps[k]), F)[0] for k in (L, R, T, B)}
    s = ((m[L] + m[R]) + m[T]) + m[B]
    m["all_div"] = np.maximum(s, F(1))
    m["all"] = np.minimum(s, F(1))
    return m


def grad_masks(h, w, overlap_w, overlap_h):
    """:181-189 with utils.lua:179-213, cast as :287 casts them (grad_masks[mode]:type(dtype)): {left, right, left_right, all} fp32 [H][W].
    The ramps are i / (n + 1) in doubles (make_gradient_mask_w_inc alone is cast to float where it is made, utils.lua:202, and back to
    double at :185: the same fp32 value in the end)."""
    gw, gh = overlap_w - 10, overlap_h - 10
    g = {k: np.zeros((h, w), np.float64) for k in (L, R, T, B)}
    g[L][:, :gw] = (np.arange(gw, 0, -1, dtype=np.float64) / (gw + 1))[None, :]                    # w_dec
    g[R][:, w - gw:] = (np.arange(1, gw + 1, dtype=np.float64) / (gw + 1)).astype(F).astype(np.float64)[None, :]      # w_inc (:float())
    g[T][:gh, :] = (np.arange(gh, 0, -1, dtype=np.float64) / (gh + 1))[:, None]                    # h_dec
    g[B][h - gh:, :] = (np.arange(1, gh + 1, dtype=np.float64) / (gh + 1))[:, None]                # h_inc
    lr = np.maximum(g[L], g[R])
    al = np.maximum(np.maximum(g[L], g[R]), np.maximum(g[T], g[B]))
    return {L: g[L].astype(F), R: g[R].astype(F), "left_right": lr.astype(F), "all": al.astype(F)}


def border(mode, last_faces, warp_fn, maps, mask_all_div, inconsistent_border, table=None):
    """:243-272: zeros for mode 0 and under -create_inconsistent_border; else the table's terms, each divided by mask_all_div (modes 4, 5)
    before it is added.  last_faces: this frame's raw faces [3][H][W], those before `mode` at least"""
    rows = (TABLE if table is None else table)[mode]
    h, w = maps[L].shape[1:]
    out = np.zeros((3, h, w), F)
    if inconsistent_border:
        return out
    for q, (src, rot, mp) in enumerate(rows):
        term = np.asarray(warp_fn(rotate(np.asarray(last_faces[src], F), rot), maps[mp]), F)
        if mode in DIVIDED:
            term = term / mask_all_div[None]
        out = term if q == 0 else out + term
    return out


def prior(mode, temporal, lfw, border_sum, cert, grads, masks):
    """:275-294.  temporal: i >= 7 and not -create_inconsistent; lfw: the previous blended face warped by the flow (:279); cert [H][W]"""
    if not temporal:
        return border_sum                                                            # :293
    if mode == 0:
        return lfw                                                                   # :285
    cert_inv = F(1) - cert                                                           # :281
    g = (grads[R], grads[L], grads["left_right"], grads["all"], grads["all"])[mode - 1]              # :282
    mk = (masks[L], masks[R], masks[L] + masks[R], masks["all"], masks["all"])[mode - 1]             # :283
    mask = np.maximum(g, np.ceil(g) * cert_inv) * mk                                 # :288
    anti = F(1) - mask                                                               # :289
    return lfw * anti[None] + border_sum * mask[None]                                # :290


def f01(u8_hwc):
    """image.load: byte / 255, [3][H][W] RGB"""
    return np.transpose(u8_hwc, (2, 0, 1)).astype(F) / F(255)


def preprocess(rgb):
    """preprocess.lua:57-62: img:index(2, {3, 2, 1}):mul(255):add(-1, mean)"""
    return rgb[::-1] * F(255) - MEAN[:, None, None]


def reflect(n, pad):
    """source index of every padded position, reflection without edge repeat (nn.SpatialReflectionPadding)"""
    i = np.arange(-pad, n + pad)
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def padded_input(frame_u8, prior_rgb, cert, fill_random, seed, i, pad):
    """core.lua:133-138 (prior_rgb None: no prior, certainty zero) and :161-171 -> [H + 2 pad][W + 2 pad][8]:
    0..2 pre(frame), 3..5 generate_fill(cert) + pre(prior) * cert, 6 cert, 7 zero (the network's eighth lane)"""
    import vr_oracle
    h, w = frame_u8.shape[:2]
    x = np.zeros((8, h, w), F)
    x[0:3] = preprocess(f01(frame_u8))                                               # :168 / :130
    c = np.zeros((h, w), F) if prior_rgb is None else np.asarray(cert, F)
    if fill_random:                                                                  # :108-117
        rnd = preprocess(vr_oracle.fill_uniform(seed, i, h, w))
        cert_inv = (c + F(-1)) * F(-1)
        x[3:6] = rnd * cert_inv[None]
    if prior_rgb is not None:
        x[3:6] = x[3:6] + preprocess(np.asarray(prior_rgb, F)) * c[None]             # :166-167, :170
    x[6] = c                                                                         # :169-171 (flow_mask is nil: -smooth_certainty off)
    yy, xx = reflect(h, pad), reflect(w, pad)
    return np.ascontiguousarray(np.transpose(x[:, yy[:, None], xx[None, :]], (1, 2, 0)))


# --------------------------------------------------------------------------------------------------------------------- inputs
def grey_certainty(h, w, seed):
    """certainty bytes: a smooth field over the whole of 0..255 plus noise, so that an erosion window still sees many different values,
    with every byte value placed somewhere"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    s = 0.5 + 0.5 * np.sin(2 * np.pi * (1.5 * x + 0.4)) * np.cos(2 * np.pi * (1.1 * y + 0.15))
    m = np.clip(np.round(s * 255 + rng.integers(-12, 13, (h, w))), 0, 255).astype(np.uint8)
    at = rng.permutation(h * w)[:256]
    m.reshape(-1)[at] = np.arange(256, dtype=np.uint8)
    return m


def fringe_flow(h, w, seed):
    """backward flow [H][W][(u, v)] of a few pixels, not on any binary grid, whose fringe leaves the face: above the first rows, right
    of the last columns, and by more than a pixel at one corner"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    ph = rng.random(4) * 2 * np.pi
    u = 3.1 * np.sin(2 * np.pi * x + ph[0]) * np.cos(2 * np.pi * y + ph[1]) + 0.37 * rng.standard_normal((h, w))
    v = 2.3 * np.cos(2 * np.pi * x + ph[2]) * np.sin(2 * np.pi * y + ph[3]) + 0.37 * rng.standard_normal((h, w))
    f = np.stack([u, v], -1).astype(F)
    f[0:2, : w // 2, 1] = F(-2.6)
    f[h // 4: h // 2, w - 2:, 0] = F(3.3)
    f[h - 1, 0] = (F(-1.25), F(4.75))
    return f


def face_values(n, seed):
    """six raw and six blended faces [3][n][n]: finite, unclamped like a network's output (some values below 0 and above 1)"""
    rng = np.random.default_rng(seed)
    raw = [(rng.standard_normal((3, n, n)) * 0.4 + 0.5).astype(F) for _ in range(6)]
    blended = [(rng.standard_normal((3, n, n)) * 0.4 + 0.5).astype(F) for _ in range(6)]
    for a in raw + blended:
        assert a.min() < 0 and a.max() > 1 and np.isfinite(a).all()
        a.setflags(write=False)
    return raw, blended


def frame_u8(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, n, 3), dtype=np.uint8)


# --------------------------------------------------------------------------------------------------------------------- one sphere, six faces
SPHERE = dict(n=64, overlap=24, ew=768, eh=384, angles=(0.842, 2.532))
# The model's worst |border - sphere_expected| per mode on sphere_faces(), over the pixels whose mask sum is positive, with vr_oracle.warp
# (tests/test_cpu_vr_input.py::test_sphere_border_per_mode prints and asserts them): what the perspective maps and the bilinear taps
# leave on a smooth image, nothing else.  The bound is TWICE the measured value; a table with one wrong entry must exceed TEN times
# the bound (test_every_single_entry_change_of_the_table_is_caught).
SPHERE_MEASURED = {1: 1.349932e-02, 2: 1.384741e-02, 3: 1.515853e-02, 4: 1.538138e-02, 5: 1.399371e-02}        # of 0..1 images
SPHERE_BOUND = {m: 2 * e for m, e in SPHERE_MEASURED.items()}


def sphere_faces(angles=None):
    """the six faces [3][64][64] (0..1) of ONE smooth image of the sphere (tests/util/equi_model.py): what a neighbour shows in the
    margin it shares with a face is what the face shows there itself.  The image is the mean of sphere_image at two angles: with one
    angle alone, whichever it is, a few wrong tables (a face's own content in place of a neighbour's, modes 4 and 5) stay below ten
    times the bound -- the image is too symmetric for them."""
    import equi_model as E
    c = SPHERE
    a, b = c["angles"] if angles is None else angles
    img = 0.5 * E.sphere_image(c["ew"], c["eh"], a).astype(np.float64) + 0.5 * E.sphere_image(c["ew"], c["eh"], b).astype(np.float64)
    _, planes = E.equi_to_faces(img, c["n"], c["n"], c["overlap"], c["overlap"], 1, np.float64)
    return [np.ascontiguousarray(np.transpose(planes[k], (2, 0, 1)) / 255.0, F) for k in range(6)]


def sphere_expected(mode, faces, masks):
    """the border of face `mode` if every warped neighbour showed exactly the face's own content under its warped-ones mask:
    own * (sum of the masks of the mode's terms) / the mode's divisor; and the pixels where that mask sum is positive"""
    s = np.zeros_like(masks[L])
    for (_, _, mp) in TABLE[mode]:
        s = s + masks[mp]
    d = masks["all_div"] if mode in DIVIDED else np.ones_like(s)
    return faces[mode] * (s / d)[None], s > 0


def table_changes(mode):
    """every table that differs from TABLE in ONE entry of face `mode`'s row: each rotation to each other rotation, each map to each
    other map, each source face to each other face -> [(description, table)]"""
    out = []
    row = TABLE[mode]
    for q, (src, rot, mp) in enumerate(row):
        alts = [(src, r, mp) for r in (ROT0, ROT90, ROTM90, ROT180) if r != rot]
        alts += [(src, rot, m) for m in (L, R, T, B) if m != mp]
        alts += [(s, rot, mp) for s in range(6) if s != src]
        for a in alts:
            t = dict(TABLE)
            t[mode] = row[:q] + (a,) + row[q + 1:]
            out.append((f"mode {mode} term {q}: {(src, rot, mp)} -> {a}", t))
    return out
