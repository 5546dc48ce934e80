"""The call scripts of tests/test_gpu_stream_history.py cannot silently cover nothing: for each committed script, which step kinds and
variants occur, which hazards its steps contain (named in the steps' tags), that it stays inside the entry points' documented preconditions
(the state machine of tests/util/stream_script.py) and that it is short.  No GPU: the generator alone.

Kinds are the entry points and the three refused calls (each at least twice); a kind's forms are its variants (each at least once).  The
script at 50 x 70 (stylised frames of 52 x 72) leaves out what fav.h rules out at that size: the scaled single-image path and the _colors
encodes."""
import copy
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import stream_script as S  # noqa: E402


def _absent(cfg):
    return (set() if cfg["scaled"] else S.SCALED_ONLY) | (set() if cfg["colors"] else S.COLORS_ONLY)


@pytest.fixture(scope="module")
def scripts():
    return S.committed_scripts()


def test_the_committed_sizes_and_options():
    by = S.SCRIPTS
    assert [c["size"] for c in by.values()].count((48, 72)) == 3 and by["larger-state-50x70"]["size"] == (50, 70)
    assert not by["larger-state-50x70"]["scaled"] and all(c["scaled"] for n, c in by.items() if n != "larger-state-50x70")
    assert by["fill-random-48x72"]["opts"] == dict(fill_random=True, seed=5)
    assert by["options-48x72"]["opts"] == dict(invert_occlusion=True, fix_occlusions=True, min_filter_r=3, border="cpu")
    assert len({c["seed"] for c in by.values()}) == len(by)


@pytest.mark.parametrize("name", list(S.SCRIPTS))
def test_script_covers_every_kind_variant_and_hazard(scripts, name):
    cfg, script = S.SCRIPTS[name], scripts[name]
    absent = _absent(cfg)
    assert len(script) <= 64, "%d steps" % len(script)
    sim = S.simulate(copy.deepcopy(script), cfg["scaled"], cfg["colors"])          # raises where a precondition is left
    kinds = [s["op"] for s in script]
    for kind in S.KINDS:
        if kind not in absent:
            assert kinds.count(kind) >= 2, "%s: %s occurs %d times" % (name, kind, kinds.count(kind))
    assert not set(kinds) & absent and set(kinds) <= set(S.KINDS)
    variants = [v for v, _, _ in sim if v]
    for v in S.VARIANTS:
        assert (v in variants) == (v not in absent), "%s: variant %s" % (name, v)
    # the hazards: found by the state machine, and named in the tag of the step they occur in
    found = {}
    for i, (step, (_, hz, _)) in enumerate(zip(script, sim)):
        assert sorted(S.hazards_of(step)) == sorted(hz), "step %d: tag %r, the state machine finds %r" % (i, step["tag"], hz)
        for h in hz:
            found.setdefault(h, []).append(i)
    for h in S.HAZARDS:
        assert (h in found) == (h not in absent), "%s: hazard %s" % (name, h)
    print("%s (seed %d): %d steps, %d stylising, %d look-aheads" % (name, cfg["seed"], len(script), sum(k in S.STYLISING for k in kinds),
                                                                    kinds.count("prefetch_mask")))
    for h in S.HAZARDS:
        for i in found.get(h, []):
            print("  %-40s step %2d  %s" % (h, i, script[i]["tag"]))


@pytest.mark.parametrize("name", list(S.SCRIPTS))
def test_look_ahead_outcomes_are_the_ones_the_script_is_about(scripts, name):
    """a hit in each mode, a miss computed inline, a hit across first_frame and one across set_state, a slot reused unconsumed"""
    script = scripts[name]
    flows = [s for s in script if s["op"] == "next_frame_flow"]
    assert sum(s["hit"] for s in flows) >= 4 and sum(not s["hit"] for s in flows) >= 2
    for restart in ("first_frame", "set_state"):
        i = next(k for k, s in enumerate(script) if "lookahead-across-" + restart in S.hazards_of(s))
        nxt = next(s for s in script[i + 1:] if s["op"] in S.STYLISING)
        assert nxt["op"] == "next_frame_flow" and nxt["hit"], "the look-ahead in flight across %s is consumed by the next frame" % restart


def test_the_state_machine_refuses_what_the_header_forbids(scripts):
    base = scripts["plain-48x72"]

    def broken(change):
        s = copy.deepcopy(base)
        change(s)
        with pytest.raises(S.ScriptError):
            S.simulate(s)

    lt = next(i for i, s in enumerate(base) if s["op"] == "next_frame_flows_lt")
    broken(lambda s: s.insert(lt, dict(op="prefetch_mask", frame=s[lt]["frame"], ahead=1, structure=False, sync=False, tag="")))   # pending at an _lt call
    broken(lambda s: s[lt].update(m=4))                                                      # more distances than the history serves
    broken(lambda s: s.pop(0))                                                               # no first frame
    host = next(i for i, s in enumerate(base) if s["op"] == "prefetch_mask" and s["sync"])
    broken(lambda s: s[host].update(sync=False))                                             # host-ordered look-ahead without the caller's synchronisation
    broken(lambda s: s.insert(1, dict(op="next_frame_estimate_lt", frame=1, structure=False, tag="")))     # long-term priors off
    with pytest.raises(S.ScriptError):
        S.simulate(copy.deepcopy(base), scaled_allowed=False)
    with pytest.raises(S.ScriptError):
        S.simulate(copy.deepcopy(base), colors_allowed=False)
