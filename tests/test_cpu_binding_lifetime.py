"""fav_amd destroys a network only after the streams / 360-degree objects built on it (no GPU needed: the library is replaced by a
recorder).  ~fav_stream and ~fav_vr read their network, and the garbage collector finalises the members of a reference cycle in any
order, so Net.close() with users left must wait for the last of them."""
import ctypes as C

import pytest


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name.endswith("_create"):
                C.cast(args[-1], C.POINTER(C.c_void_p))[0] = C.c_void_p(0x1000 + len(self.calls))
            return 0
        return call


@pytest.fixture()
def rec(monkeypatch):
    import fav_amd
    r = _Recorder()
    monkeypatch.setattr(fav_amd, "lib", lambda: r)
    return fav_amd, r


def _destroys(r):
    return [c for c in r.calls if c.endswith("_destroy")]


def test_net_closed_first_is_destroyed_last(rec):
    fav, r = rec
    net, img = fav.Net("m.t7"), fav.Net("i.t7")
    st = fav.Stream(net, 8, 8)
    st.set_image_net(img)
    vr = fav.VR(net, 32, 32, image_net=img)
    net.close(); img.close()
    assert _destroys(r) == [] and net.h and img.h
    st.close()
    assert _destroys(r) == ["fav_stream_destroy"]
    vr.close()
    assert _destroys(r) == ["fav_stream_destroy", "fav_vr_destroy", "fav_net_destroy", "fav_net_destroy"]
    assert net.h is None and img.h is None
    for o in (st, vr, net, img):
        o.close()                                    # idempotent
    assert len(_destroys(r)) == 4


def test_usual_order_and_finalisers(rec):
    fav, r = rec
    net = fav.Net("m.t7")
    st = fav.Stream(net, 8, 8)
    st.close(); net.close()
    assert _destroys(r) == ["fav_stream_destroy", "fav_net_destroy"]
    r.calls.clear()
    net = fav.Net("m.t7")
    st = fav.Stream(net, 8, 8)
    net.__del__()                                    # the collector ran the network's finaliser first
    assert _destroys(r) == []
    st.__del__()
    assert _destroys(r) == ["fav_stream_destroy", "fav_net_destroy"]
    r.calls.clear()
    a, b = fav.Net("a.t7"), fav.Net("b.t7")
    st = fav.Stream(net := fav.Net("m.t7"), 8, 8)
    st.set_image_net(a); st.set_image_net(b); a.close()          # replaced: a is free to go at once
    assert _destroys(r) == ["fav_net_destroy"]
    b.close(); st.close(); net.close()
    assert _destroys(r) == ["fav_net_destroy", "fav_stream_destroy", "fav_net_destroy", "fav_net_destroy"]
