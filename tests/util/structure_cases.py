"""Sizes and images of the structure-map tests (tests/test_cpu_structure.py, tests/test_gpu_structure.py, the recipe of
tests/golden/structure_ref_cases.npz in tests/golden/make_golden.py).

The sizes come from the kernels (csrc/kernels_consistency.hip), not from the workload.  A line of the recursive passes has n = W
samples in the X pass and n = H in the Y pass; the LDS ring is D = 22 deep in the wide form and D = 14 in the packed one; a lane
carries 4 lines, a wave 256.  Sizes are (H, W)."""
import numpy as np

from fav_amd import synth

RING_WIDE, RING_PACKED = 22, 14

# n in {2, 3, D-1, D, D+1, 2D-1, 2D, 2D+1} for both ring depths, on both axes
RING_SIZES = [(2, 2), (2, 3), (3, 2), (13, 14), (14, 13), (14, 15), (15, 27), (27, 28), (28, 29), (21, 22), (22, 21), (22, 23),
              (43, 44), (44, 45), (45, 71)]
# line counts around a wave of 256 lines (one active lane in the last group, a group of four that hangs over the row pitch)
WAVE_SIZES = [(255, 30), (256, 29), (257, 28), (261, 45), (30, 255), (29, 256), (28, 257), (45, 261), (513, 23), (23, 513)]
# the sequential sum's hand-over at 65 536 values: one block / the first multi-chunk length / above it
SUM_SIZES = [(255, 257), (256, 256), (301, 258), (130, 1029)]
SIZES = RING_SIZES + WAVE_SIZES + SUM_SIZES
# the full cross pack_cus x q0 of the packed form
CROSS_SIZES = [(14, 15), (45, 261), (257, 28), (301, 258)]
# one size of each group: run again behind NaN-filled LDS
POISON_SIZES = [(22, 23), (261, 45), (256, 256)]

KINDS = ["smooth", "noise", "const", "half", "pixel"]

# the committed fixture (recorded results of the reference's compiled code): every kind at the sizes below 32x32 (they carry the
# weight: first / last samples, lines around both ring depths), three kinds at two larger sizes (the file stays below 300 KB)
FIXTURE_CASES = [(h, w, k) for (h, w) in RING_SIZES[:12] + [(5, 4), (31, 33)] for k in KINDS] + \
                [(h, w, k) for (h, w) in [(44, 45), (64, 96)] for k in ("smooth", "half", "pixel")]


def image(kind: str, h: int, w: int) -> np.ndarray:
    """u8 [H][W][3], a function of (kind, h, w) alone"""
    seed = 1000 * h + w
    if kind == "smooth":
        return synth.smooth_frame(h, w, seed)
    if kind == "noise":
        return synth.random_frame(h, w, seed + 1)
    if kind == "const":
        return np.full((h, w, 3), 77, np.uint8)
    if kind == "half":                       # left half black
        a = synth.random_frame(h, w, seed + 2)
        a[:, :w // 2] = 0
        return a
    if kind == "pixel":                      # one white pixel on black: a map that is almost all zeros
        a = np.zeros((h, w, 3), np.uint8)
        a[h // 3, (2 * w) // 3] = 255
        return a
    raise ValueError(kind)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got_map, got_avg, want_map, want_avg, label: str = "", ring=(RING_WIDE, RING_PACKED)) -> None:
    """equality of the uint32 views of the maps and of the averages' four bytes; the message points at a round, a tail or a group"""
    g, w = bits(got_map), bits(want_map)
    assert g.shape == w.shape, (label, g.shape, w.shape)
    ga, wa = np.float32(got_avg).tobytes(), np.float32(want_avg).tobytes()
    bad = np.argwhere(g != w)
    if len(bad) == 0 and ga == wa:
        return
    msg = [f"{label}: structure map {g.shape[0]}x{g.shape[1]} (HxW)"]
    if len(bad):
        with np.errstate(invalid="ignore"):
            d = np.abs(np.asarray(got_map, np.float64) - np.asarray(want_map, np.float64))
        y, x = (int(v) for v in bad[0])
        msg.append(f"{len(bad)} of {g.size} values differ, max |diff| {np.nanmax(d[g != w]) if np.isfinite(d[g != w]).any() else float('nan'):.3e}"
                   f" ({int(np.isnan(np.asarray(got_map)[g != w]).sum())} of them NaN)")
        msg.append(f"first at (y, x) = ({y}, {x}): got {np.asarray(got_map)[y, x]!r} (0x{g[y, x]:08x}) want {np.asarray(want_map)[y, x]!r} (0x{w[y, x]:08x})")
        for name, n, lines in (("X pass (sample x, line y)", x, y), ("Y pass (sample y, line x)", y, x)):
            msg.append(f"  {name}: sample mod ring depth " + ", ".join(f"{n % D} (D={D})" for D in ring) +
                       f"; line mod 256 = {lines % 256}, line mod 4 = {lines % 4}")
        ys, xs = bad[:, 0], bad[:, 1]
        msg.append(f"  rows {ys.min()}..{ys.max()}, columns {xs.min()}..{xs.max()}")
    if ga != wa:
        msg.append(f"average: got {np.float32(got_avg)!r} ({ga.hex()}) want {np.float32(want_avg)!r} ({wa.hex()})")
    raise AssertionError("\n".join(msg))
