"""numpy restatement of csrc/kernels_color.hip ("Original colours"): the stylised frame's luminance on the original frame's
colours.  S = image.save's bytes of the stylised planes, O = the original frame's bytes; per pixel, in this order:

    ys = (Kr Sr + Kg Sg) + Kb Sb;  yo = (Kr Or + Kg Og) + Kb Ob;  d = ys - yo;  Pc = clamp(floor((Oc + d) + 0.5), 0, 255), c = R, G, B

with dtype=np.float32 every operation rounds like the kernels' (the unit is compiled without FMA contraction), so they are held to this
model byte for byte; dtype=np.float64 is the same arithmetic with unrounded constants: the yardstick of the fp32 model.  The planes of the
Y4M route are yuv_model.rgb_to_yuv of P's bytes -- that file's function, not a second copy."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_model as Y  # noqa: E402


def luma(rgb_hwc, matrix, dtype=np.float32):
    """(Kr R + Kg G) + Kb B of bytes [H][W][3], unquantised, full range"""
    k = Y.constants(Y.Format("444", "center", matrix, True), dtype)
    R, G, B = (np.asarray(rgb_hwc)[..., c].astype(dtype) for c in range(3))
    return (k["kr"] * R + k["kg"] * G) + k["kb"] * B


def transfer_unquantised(S_hwc, O_hwc, matrix, dtype=np.float32):
    """O + d before rounding and clamping, [H][W][3] in dtype"""
    d = luma(S_hwc, matrix, dtype) - luma(O_hwc, matrix, dtype)
    return np.asarray(O_hwc).astype(dtype) + d[..., None]


def transfer_bytes(S_hwc, O_hwc, matrix, dtype=np.float32):
    """P from the stylised frame's BYTES S and the original's bytes O, both [H][W][3] u8"""
    return Y.quantise(transfer_unquantised(S_hwc, O_hwc, matrix, dtype))


def transfer(state_planar, O_hwc, matrix, dtype=np.float32):
    """P from the state's planes [3][H][W] fp32 (image.save's quantisation in front) and O"""
    return transfer_bytes(Y.quantise_f32_image(state_planar), O_hwc, matrix, dtype)


def transfer_yuv(state_planar, O_hwc, fmt, dtype=np.float32):
    """the Y4M payload: the conversion of P's bytes; the transfer takes the format's matrix"""
    return Y.rgb_to_yuv(transfer(state_planar, O_hwc, fmt.matrix, dtype), fmt, dtype)
