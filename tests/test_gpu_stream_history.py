"""A long-lived Stream against Streams without history, bit for bit (csrc/stream.cpp: the state buffers that trade places under the
asynchronous encoder, the look-ahead slots, host-ordered mode, the long-term ring, the scaled single-image path, the frame counter).

One subject Stream is driven through a script that mixes every feature (tests/util/stream_script.py; what each script contains is held
by tests/test_cpu_stream_script.py).  After every stylising step its returned frames, state(), last_mask(), last_input(),
last_padded_input() and long_term_available() are those of a twin that has no history:
  * a fresh Stream on the same Net given set_state(the subject's state before the step) and the same call in its plainest form;
  * for the long-term steps, favlib.long_term_input + Net.forward on the states, frames and flows the runner recorded itself;
  * with fill_random (the fill is keyed by the frame counter) a second long-lived Stream that receives the stylising calls alone.
After every encoding step the bytes are those of the same encode on a fresh Stream holding the same state.  The twins get fresh device
copies of every input, so nothing keyed by a pointer agrees by accident.  No tolerance anywhere: torch.equal on the words."""
import os
import sys

import pytest

from fav_amd import t7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "util"))
import stream_script as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets(favlib, golden_dir, tmp_path_factory):
    """the video model, and an image model of its layout (3 input channels, the same padding and output sizes)"""
    path = str(tmp_path_factory.mktemp("stream_history") / "img.t7")
    t7.make_synthetic_checkpoint(path, arch="c9s1-8,d16,d32,R32,R32,U2,c3s1-16,U2,c9s1-3", seed=5, in_channels=3)
    net, img = favlib.Net(os.path.join(golden_dir, "tiny_model.t7"), 0), favlib.Net(path, 0)
    yield net, img
    net.close(); img.close()


@pytest.fixture(scope="module")
def scripts():
    return S.committed_scripts()


def _run(favlib, cuda, nets, scripts, name):
    stats = S.Runner(favlib, nets[0], nets[1], name, scripts[name], cuda).run()
    print("%s: %d steps, %d Streams, %d values / %d bytes compared" % (name, stats["steps"], stats["twins"], stats["values"], stats["bytes"]))


@pytest.mark.parametrize("name", list(S.SCRIPTS))
def test_every_call_equals_its_twin_without_history(favlib, cuda, nets, scripts, name):
    _run(favlib, cuda, nets, scripts, name)


def test_every_call_equals_its_twin_on_dirty_memory(favlib, cuda, nets, scripts, poison):
    """the same 48 x 72 script with LDS and freed device memory holding NaN: what the subject allocates mid-script (the PNG workspace, the
    second state buffer, color_rgb8, the scaled pair, the history ring, the long-term masks and certainties) is allocated dirty"""
    poison()
    _run(favlib, cuda, nets, scripts, "plain-48x72")


@pytest.mark.parametrize("kind", S.REFUSED)
def test_a_refused_call_changes_nothing(favlib, cuda, nets, kind):
    """state(), last_mask(), long_term_available() and the next stylising step with the refused call in between are those without it"""
    import torch
    net, h, w = nets[0], 48, 72
    frames, bws, fws = S.make_clip(h, w, 4, 77)
    T = lambda a: torch.from_numpy(a).to(cuda)
    fr, bw, fw = [T(f) for f in frames], [None] + [T(b) for b in bws[1:]], [None] + [T(f) for f in fws[1:]]
    far = [T(x) for x in S.far_flows(h, w, 3, 2, 77)]
    seen = []
    for refuse in (False, True):
        st = favlib.Stream(net, h, w, fill_random=True, seed=5)      # (the fill is keyed by the frame counter: a counter that moved shows)
        st.set_long_term((1, 2))
        st.first_frame(fr[0])
        st.next_frame_flow(fr[1], bw[1], fw[1], use_structure=True)
        st.next_frame_flows_lt(fr[2], [bw[2]], [fw[2]])
        if refuse:
            with pytest.raises(favlib.FavError):
                if kind == "refuse_lt_distances":
                    st.first_frame(fr[0]); st.next_frame_flows_lt(fr[1], [bw[1], far[0]], [fw[1], far[1]])
                else:
                    bad = kind == "refuse_flow_option"
                    S.estimate_raw(favlib, st, fr[3], fr[2], dict(S.FLOW_OPTS, median=4) if bad else S.FLOW_OPTS, 0 if bad else -256)
        elif kind == "refuse_lt_distances":
            st.first_frame(fr[0])                                    # (the restart that makes two distances too many is in both runs)
        after = [st.state(), st.last_mask(), st.long_term_available()]
        m = st.long_term_available()
        f, u = st.next_frame_flows_lt(fr[3], [bw[3], far[0]][:m], [fw[3], far[1]][:m], use_structure=True, want_u8=True)
        seen.append(after + [f, u, st.last_padded_input(), st.long_term_available()])
        st.close()
    names = ("state()", "last_mask()", "long_term_available()", "the next f32 frame", "the next u8 frame", "the next padded input",
             "long_term_available() after the next frame")
    for name, a, b in zip(names, *seen):
        assert (a == b) if isinstance(a, int) else S.bits_equal(a, b), "%s: %s differs with the refused call in between" % (kind, name)
