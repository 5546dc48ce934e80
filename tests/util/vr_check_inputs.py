"""Inputs of the cube-map consistency-check tests (tests/test_cpu_vr_check.py, tests/test_gpu_vr_check.py): two frames of six faces,
the fixture recipe of test_gpu_vr.py::test_vr_two_frames_vs_oracle (smooth frames, synth backward flows) plus the forward flow the
flat-path tests derive from the backward one.  numpy only."""
import numpy as np

from fav_amd import synth

HP = 64            # face size (hplus = wplus)
OVERLAP = 24
SEED = 300         # the faces' masks at this seed are neither all 0 nor all 255: test_cpu_vr_check.py checks that on the oracle
NOISE = 0.75       # px of noise on the forward flow: around the checker's threshold (0.5 + 1 % of the motion), so both byte values occur


def face_inputs(hp=HP, wp=HP, frames=2, seed=SEED):
    """[(i, frame u8 [H][W][3], backward flow | None, forward flow | None)] in processing order; flows from the second frame on"""
    out = []
    for fr in range(frames):
        for mode in range(6):
            i = fr * 6 + mode + 1
            f = synth.smooth_frame(hp, wp, seed + i)
            bw = fw = None
            if i >= 7:
                bw = synth.backward_flow(hp, wp, seed + 50 + i)
                fw = synth.forward_flow_from_backward(bw, seed + 100 + i, noise=NOISE)
            out.append((i, f, bw, fw))
    return out


def reliable_fraction(mask):
    return float(np.count_nonzero(mask == 255)) / mask.size
