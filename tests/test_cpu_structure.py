"""The structure map of the 4-argument consistency check (computeCorners + CMatrix::normalize(0, 1) + CMatrix::avg,
consistencyChecker.cpp:39-78,158-159), value by value: the oracle's map (oracle.structure: fp32 operations in the reference's order)
against the reference's OWN compiled code, bit for bit -- uint32 views of the maps, the average as four bytes, no tolerance.

The reference's code is reached through oracle/structure_ref_shim.cpp, which includes the reference's consistencyChecker.cpp at build
time (oracle/Makefile, target structure_ref: g++ -O3 -fPIC -w -shared, the reference's own flags) and repeats the four statements of its
main() that make the map.  Where the reference tree is absent its recorded results stand in: tests/golden/structure_ref_cases.npz
(recipe: tests/golden/make_golden.py --structure).  tests/test_gpu_structure.py holds the GPU kernels to the same maps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import structure_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, "structure_ref_cases.npz"))


def test_fixture_holds_the_recipe_inputs(recorded):
    """the images in the fixture are the ones tests/util/structure_cases.py makes today (the GPU tests regenerate them)"""
    assert len(recorded.files) == 3 * len(SC.FIXTURE_CASES)
    for (h, w, kind) in SC.FIXTURE_CASES:
        assert np.array_equal(recorded[f"img_{h}x{w}_{kind}"], SC.image(kind, h, w)), (h, w, kind)


def test_fixture_reaches_the_odd_corners(recorded):
    """what the recorded maps contain: minima below 0 (normalize's else-if scan misses a minimum that is also a running maximum),
    values above 1 (a map that only rises in scan order never updates the minimum: it stays at +30000), all-zero maps with average +0
    (flat frames), nothing that is not finite"""
    below, above, flat = 0, 0, 0
    for (h, w, kind) in SC.FIXTURE_CASES:
        m, avg = recorded[f"map_{h}x{w}_{kind}"], recorded[f"avg_{h}x{w}_{kind}"]
        assert m.shape == (h, w) and m.dtype == np.float32 and np.isfinite(m).all() and np.isfinite(avg), (h, w, kind)
        if kind == "const":
            assert not SC.bits(m).any() and np.float32(avg).tobytes() == np.float32(0).tobytes(), (h, w)
            flat += 1
        below += bool(m.min() < 0); above += bool(m.max() > 1)
    assert below >= 5 and above >= 1 and flat >= 10, (below, above, flat)


@pytest.mark.parametrize("case", SC.FIXTURE_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_oracle_structure_map_is_the_recorded_reference_map(oracle, recorded, case):
    h, w, kind = case
    m, avg = oracle.structure(recorded[f"img_{h}x{w}_{kind}"])
    SC.same_bits(m, avg, recorded[f"map_{h}x{w}_{kind}"], recorded[f"avg_{h}x{w}_{kind}"], f"oracle vs recorded reference, {kind}")


@pytest.mark.parametrize("size", SC.SIZES + [(64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_structure_map_is_the_live_reference_map(oracle, size):
    """every size of the GPU tests, every image kind, against the reference's compiled code itself -- and finite everywhere, which the
    GPU tests rely on when they compare bits"""
    if not oracle.structure_ref_available():
        pytest.skip("oracle/_ref/libstructure_ref.so is not built (no reference tree on this machine): the recorded cases stand in")
    h, w = size
    for kind in SC.KINDS:
        img = SC.image(kind, h, w)
        m, avg = oracle.structure(img)
        rm, ravg = oracle.structure_ref(img)
        assert np.isfinite(m).all() and np.isfinite(avg), (h, w, kind)
        SC.same_bits(m, avg, rm, ravg, f"oracle vs live reference, {kind}")


def test_recorded_cases_are_what_the_live_reference_gives(oracle, recorded):
    if not oracle.structure_ref_available():
        pytest.skip("oracle/_ref/libstructure_ref.so is not built (no reference tree on this machine)")
    for (h, w, kind) in SC.FIXTURE_CASES:
        rm, ravg = oracle.structure_ref(recorded[f"img_{h}x{w}_{kind}"])
        SC.same_bits(recorded[f"map_{h}x{w}_{kind}"], recorded[f"avg_{h}x{w}_{kind}"], rm, ravg, f"recorded vs live reference, {kind}")


def test_consistency_takes_a_map_from_outside(oracle, golden_dir):
    """consistency(..., structure=) with the oracle's own map is consistency(..., rgb)"""
    g = np.load(os.path.join(golden_dir, "mask_smooth_64x96.npz"))
    m, _ = oracle.structure(g["img"])
    assert np.array_equal(oracle.consistency(g["bw"], g["fw"], structure=m), g["mask4"])
    assert np.array_equal(oracle.consistency(g["bw"], g["fw"], g["img"]), g["mask4"])


def test_a_wrong_line_start_is_invisible_in_the_mask_and_plain_in_the_map(oracle, golden_dir):
    """The gap the value-by-value tests close.  The first 14 samples of one row of the map (a first round of the packed form's ring)
    scaled by 1 + 1e-3 -- the size of error a mishandled line start leaves -- move NO byte of the 4-argument mask: the map reaches the
    mask only through one comparison per pixel (4 / avg * max(0, avg / 2 - s) against a squared forward-backward error), which flips
    only where that error lies within the perturbation of the threshold.  The comparison of values reports exactly those 14 samples.
    Row 20 of mask_smooth_64x96.npz (chosen as a row whose samples all differ after the scaling; the mask stays byte-identical)."""
    g = np.load(os.path.join(golden_dir, "mask_smooth_64x96.npz"))
    m, avg = oracle.structure(g["img"])
    row = 20
    wrong = m.copy()
    wrong[row, :14] = m[row, :14] * np.float32(1 + 1e-3)
    changed = np.argwhere(SC.bits(wrong) != SC.bits(m))
    assert len(changed) == 14 and (changed[:, 0] == row).all() and list(changed[:, 1]) == list(range(14))
    # the sequential average moves too (or not, at this size of error): it is taken from the wrong map, as a wrong kernel would
    assert np.array_equal(oracle.consistency(g["bw"], g["fw"], structure=wrong), g["mask4"])
    with pytest.raises(AssertionError) as e:
        SC.same_bits(wrong, avg, m, avg, "perturbed")
    text = str(e.value)
    assert "14 of 6144 values differ" in text and f"first at (y, x) = ({row}, 0)" in text and f"rows {row}..{row}, columns 0..13" in text
