"""Host side of the 360-degree path's on-device consistency check (no GPU needed): the flags of fav_stylize_vr, the exported symbols,
the Python binding, and the premise of tests/test_gpu_vr_check.py's mask comparisons (masks that are neither all 0 nor all 255)."""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "util"))
import vr_check_inputs as VI  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fast-artistic-videos_amd", "bin", "fav_stylize_vr")
BASE = [EXE, "-input_pattern", "v/%S/f_%05d-%d.ppm", "-model_vid", "m.t7", "-output_prefix", "o/%S/out"]
BW = ["-flow_pattern", "v/%S/flow-%d/backward_[%d]_{%d}.flo"]
FW = ["-forward_flow_pattern", "v/%S/flow-%d/forward_{%d}_[%d].flo"]
OCC = ["-occlusions_pattern", "v/%S/flow-%d/reliable_[%d]_{%d}.pgm"]


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=60)


def test_forward_flow_pattern_is_an_option_and_replaces_the_certainty_files(favlib):
    """-forward_flow_pattern is accepted, makes -occlusions_pattern optional, and goes through the -streams / -gpus launcher with %S"""
    r = _run(BASE + BW + FW + ["-gpu", "2", "-streams", "x,y,z", "-gpus", "2", "-dry_run", "1"])
    assert r.returncode == 0, r.stderr
    assert "unknown option" not in r.stderr and "Must give" not in r.stderr
    recs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda d: d["rank"])
    assert [[s["name"] for s in d["streams"]] for d in recs] == [["x", "z"], ["y"]]
    assert recs[1]["streams"][0]["forward_flow_pattern"] == "v/y/flow-%d/forward_{%d}_[%d].flo"
    assert recs[1]["streams"][0]["flow_pattern"] == "v/y/flow-%d/backward_[%d]_{%d}.flo"
    # -structure 0 | 1 are values of the new flag; the option set ends where it did (no device: it gets as far as the backend check)
    for s in ("0", "1"):
        r = _run(BASE + BW + FW + ["-structure", s, "-gpu", "-1"])
        assert r.returncode != 0 and "no CPU backend" in r.stderr, r.stderr


def test_both_patterns_given_the_forward_flow_wins(favlib):
    r = _run(BASE + BW + FW + OCC + ["-gpu", "0", "-dry_run", "1"])
    assert r.returncode == 0 and "the forward flow wins" in r.stderr, r.stderr
    r = _run(BASE + BW + OCC + ["-gpu", "0", "-dry_run", "1"])
    assert r.returncode == 0 and "wins" not in r.stderr


def test_structure_takes_0_or_1(favlib):
    for bad in ("2", "-1", "yes", ""):
        r = _run(BASE + BW + FW + ["-structure", bad, "-gpu", "0", "-dry_run", "1"])
        assert r.returncode != 0 and "-structure must be 0 or 1" in r.stderr, (bad, r.stderr)


def test_flow_pattern_is_still_required(favlib):
    """the reference's message (fast_artistic_video_vr.lua:567-569)"""
    r = _run(BASE + FW + ["-gpu", "0", "-dry_run", "1"])
    assert r.returncode != 0 and "Must give -flow_pattern and -occlusions_pattern" in r.stderr
    r = _run(BASE + BW + ["-gpu", "0", "-dry_run", "1"])                  # neither certainty source
    assert r.returncode != 0 and "Must give -flow_pattern and -occlusions_pattern" in r.stderr


def test_library_exports_and_binding(favlib):
    out = subprocess.run(["nm", "-D", "--defined-only", favlib.LIB_PATH], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in ("fav_vr_face_flow", "fav_vr_prefetch_mask", "fav_vr_last_mask"):
        assert name in defined, name
        assert name in favlib.EXPORTS
        getattr(favlib.lib(), name)
    for method in ("face_flow", "prefetch_mask", "last_mask"):
        assert callable(getattr(favlib.VR, method))
    assert favlib.lib().fav_vr_last_mask(None) is None                  # null handle: a null pointer, not a crash
    import inspect
    assert "5:" in inspect.getsource(favlib.VR.get)                    # get(5): the certainty plane


def test_masks_of_the_gpu_tests_are_not_vacuous(oracle):
    """every mask tests/test_gpu_vr_check.py compares has between 10 % and 90 % of its bytes at 255 -- on the ORACLE's checker,
    3- and 4-argument mode, both face sizes used there"""
    seen = 0
    for hp in (VI.HP, 76):
        for (i, f, bw, fw) in VI.face_inputs(hp, hp):
            if bw is None:
                continue
            m3, m4 = oracle.consistency(bw, fw), oracle.consistency(bw, fw, f)
            for m in (m3, m4):
                assert set(np.unique(m)) <= {0, 255}
                assert 0.10 <= VI.reliable_fraction(m) <= 0.90, (hp, i, VI.reliable_fraction(m))
            if hp == VI.HP:
                seen += int((m3 != m4).any())
    assert seen >= 1                                                   # the structure term decides pixels: the two modes differ
