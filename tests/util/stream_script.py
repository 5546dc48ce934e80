"""Call scripts over one long-lived fav_stream, and the twins without history that every call is held to (tests/test_gpu_stream_history.py;
the coverage of the scripts themselves: tests/test_cpu_stream_script.py).  Importing this module needs no GPU.

A script is a list of steps (dicts: op, tag, arguments) over one synthetic clip.  build_script() writes the committed scripts: the skeleton
is explicit -- every hazard below is placed by hand -- and the seed varies what the skeleton leaves open (the structure flags, the YUV
formats, the long-term distances, which recorded state set_state restores).  simulate() is a small state machine over the stream's
documented state (include/fav.h, include/fav_long_term.h): it refuses a script that leaves an entry point's preconditions and names the
hazards each step contains; annotate() writes those names into the steps' tags.  run_script() drives the subject and the twins on the GPU.

Step kinds are the entry points (and the three refused calls); a kind's forms (plain / image model / scaled first frame, 3- / 4-argument
check, single / pairs workspace, one / two frames ahead, with / without wait_png, on / changed / off) are its variants."""
import os
import sys

import numpy as np

NPREF = 4                                    # look-ahead slots of a stream, dealt round-robin (csrc/stream.cpp)
SCALED_SIZE = (40, 60)                       # set_single_image_size: larger than tiny_model.t7's padding of 16, another aspect than the frames
FLOW_OPTS = dict(warps=2, iters=10)          # the estimator of the next_frame_estimate* steps: small, the test is about the stream

STYLISING = ("first_frame", "next_frame_cert", "next_frame_flow", "next_frame_estimate", "next_frame_flows_lt", "next_frame_estimate_lt")
ENCODING = ("encode_png", "encode_png_async", "encode_yuv", "encode_yuv_layout", "encode_png_colors", "encode_yuv_colors")
MODES = ("set_state", "set_host_ordered", "set_long_term", "set_single_image_size", "set_image_net")
REFUSED = ("refuse_flow_option", "refuse_small_workspace", "refuse_lt_distances")
KINDS = STYLISING + ("prefetch_mask",) + ENCODING + MODES + REFUSED
VARIANTS = ("first_frame:plain", "first_frame:image_net", "first_frame:scaled", "next_frame_flow:3", "next_frame_flow:4",
            "next_frame_estimate:single", "next_frame_estimate:pairs", "prefetch_mask:+1", "prefetch_mask:+2",
            "encode_png_async:wait", "encode_png_async:nowait", "set_host_ordered:on", "set_host_ordered:off",
            "set_long_term:on", "set_long_term:changed", "set_long_term:off", "set_single_image_size:on", "set_single_image_size:off",
            "set_image_net:on", "set_image_net:off")
HAZARDS = ("async-pending@set_state", "async-pending@first_frame", "async-pending@long-term", "lookahead-miss",
           "unconsumed-lookahead-slot-reused", "lookahead-across-first_frame", "lookahead-across-set_state",
           "host-hit-after-event-hit", "history-ring-wraps", "set_state-then-lt-one-frameless-entry",
           "scaled-first-then-last_input", "refused-between-stylising")
SCALED_ONLY = {"set_single_image_size", "first_frame:scaled", "set_single_image_size:on", "set_single_image_size:off",
               "scaled-first-then-last_input"}
COLORS_ONLY = {"encode_png_colors", "encode_yuv_colors"}

# the committed scripts: (name, seed, frame size, Stream options, what the size rules out)
SCRIPTS = {
    "plain-48x72": dict(seed=11, size=(48, 72), opts={}, scaled=True, colors=True),
    # Ho x Wo = 52 x 72: the scaled path (fav.h: Ho == H) and the _colors encodes (fav.h: FAV_EUNSUPPORTED) do not exist at this size
    "larger-state-50x70": dict(seed=12, size=(50, 70), opts={}, scaled=False, colors=False),
    "fill-random-48x72": dict(seed=13, size=(48, 72), opts=dict(fill_random=True, seed=5), scaled=True, colors=True),
    "options-48x72": dict(seed=14, size=(48, 72), opts=dict(invert_occlusion=True, fix_occlusions=True, min_filter_r=3, border="cpu"),
                          scaled=True, colors=True),
}


class ScriptError(AssertionError):
    pass


# ================================================================================================================== the generator
class _Builder:
    def __init__(self, seed, scaled, colors):
        self.rng = np.random.default_rng(seed)
        self.steps, self.cursor, self.stylised = [], 0, 0
        self.scaled, self.colors = scaled, colors

    def flag(self):
        return bool(self.rng.integers(0, 2))

    def add(self, op, **kw):
        self.steps.append(dict(op=op, tag="", **kw))

    def frame(self, op, **kw):               # a stylising step takes the clip's next frame
        self.add(op, frame=self.cursor, **kw)
        self.cursor += 1; self.stylised += 1

    def pre(self, ahead, structure, host=False):
        self.add("prefetch_mask", frame=self.cursor - 1 + ahead, ahead=ahead, structure=structure, sync=host)

    def enc(self, op, **kw):
        if op in COLORS_ONLY and not self.colors:
            return
        if op in ("encode_yuv", "encode_yuv_colors"):
            kw.update(chroma=int(self.rng.integers(0, 2)), matrix=int(self.rng.integers(0, 2)), full_range=self.flag())
        if op == "encode_yuv_layout":
            kw.update(depth=int(self.rng.choice([8, 10, 16])), matrix=int(self.rng.integers(0, 2)))
        if op == "encode_png_colors":
            kw.update(matrix=int(self.rng.integers(0, 2)))
        if op in COLORS_ONLY:
            kw.update(frame=self.cursor - 1)
        self.add(op, **kw)


def build_script(seed, scaled=True, colors=True):
    b = _Builder(seed, scaled, colors)
    s = b.flag()
    # ---- look-aheads, encodes and restarts on the plain path (event-ordered)
    b.frame("first_frame")
    b.pre(1, not s)                                        # asked for with the other flag: missed, never consumed, its slot comes round again
    b.frame("next_frame_flow", structure=s)
    b.enc("encode_png")
    b.pre(2, True)
    b.frame("next_frame_cert")
    b.enc("encode_png_async", wait=True)
    b.frame("next_frame_flow", structure=True)             # hit, two frames after the look-ahead
    b.enc("encode_yuv")
    b.frame("next_frame_estimate", structure=b.flag(), batched=False)
    b.add("refuse_flow_option", frame=b.cursor)
    b.frame("next_frame_estimate", structure=b.flag(), batched=True)
    b.enc("encode_yuv_layout")
    b.pre(2, False)
    b.enc("encode_png_async", wait=False)
    b.add("set_image_net", on=True)
    b.frame("first_frame")                                 # the encoder still reads the state; a look-ahead is in flight
    b.frame("next_frame_flow", structure=False)            # hit across the restart
    b.enc("encode_png_colors")
    s = b.flag()
    b.pre(1, s)
    b.enc("encode_png_async", wait=False)
    b.add("set_state", source=int(b.rng.integers(0, 3)))   # the encoder still reads the state; a look-ahead is in flight
    b.frame("next_frame_flow", structure=s)                # hit across set_state
    b.enc("encode_yuv_colors")
    s = b.flag()
    b.pre(1, s)                                            # the fourth look-ahead after the missed one: takes its slot
    b.pre(2, True)
    b.frame("next_frame_flow", structure=s)                # event-ordered hit
    b.add("set_host_ordered", on=True, sync=True)          # (drops the look-ahead two frames ahead)
    b.pre(1, True, host=True)
    b.frame("next_frame_flow", structure=True)             # host-ordered hit directly after the event-ordered one
    b.add("refuse_small_workspace", frame=b.cursor)
    b.add("set_host_ordered", on=False, sync=True)
    # ---- the scaled single-image path and the image model
    if scaled:
        b.add("set_single_image_size", on=True)
    b.frame("first_frame")                                 # scaled, image model
    b.add("set_image_net", on=False)
    b.enc("encode_yuv")
    b.frame("first_frame")                                 # scaled, the video model itself
    b.frame("next_frame_cert")                             # the frame after a scaled one reads in8, not scaled_in8
    if scaled:
        b.add("set_single_image_size", on=False)
    b.enc("encode_png_colors")
    # ---- long-term priors
    far = int(b.rng.integers(3, 5))
    b.add("set_long_term", dists=(1, 2), variant="on")
    b.frame("next_frame_flows_lt", m=1, structure=b.flag())
    b.frame("next_frame_flows_lt", m=2, structure=b.flag())
    b.enc("encode_png_async", wait=False)
    b.frame("next_frame_estimate_lt", structure=b.flag())  # the encoder still reads the state
    b.add("refuse_lt_distances", frame=b.cursor, m=3)
    b.enc("encode_yuv_layout")
    b.add("set_long_term", dists=(1, far), variant="changed")
    b.frame("next_frame_flows_lt", m=1, structure=b.flag())
    b.add("refuse_flow_option", frame=b.cursor)
    b.frame("next_frame_estimate_lt", structure=b.flag())
    for _ in range(far - 2):
        b.frame("next_frame_flows_lt", m=1, structure=False)
    b.frame("next_frame_flows_lt", m=2, structure=b.flag())     # the push that wraps the ring of `far` entries
    b.enc("encode_yuv_colors")
    b.add("set_state", source=int(b.rng.integers(3, 8)))
    b.frame("next_frame_flows_lt", m=1, structure=b.flag())     # the history is the one entry set_state made, which has no frame
    b.add("refuse_lt_distances", frame=b.cursor, m=2)           # configured, but the history serves one
    b.frame("next_frame_estimate_lt", structure=b.flag())
    b.add("refuse_small_workspace", frame=b.cursor)
    b.enc("encode_png")
    b.add("set_long_term", dists=(), variant="off")
    b.frame("next_frame_flow", structure=b.flag())
    return annotate(b.steps, scaled, colors)


def committed_scripts():
    return {name: build_script(c["seed"], c["scaled"], c["colors"]) for name, c in SCRIPTS.items()}


def variant_of(step, st=None):
    """the variant a step is (None: its kind has none); first_frame's depends on the modes in force, which simulate() passes in"""
    op = step["op"]
    if op == "first_frame":
        return None if st is None else "first_frame:" + ("scaled" if st["scaled"] else "image_net" if st["img"] else "plain")
    if op == "next_frame_flow": return "next_frame_flow:" + ("4" if step["structure"] else "3")
    if op == "next_frame_estimate": return "next_frame_estimate:" + ("pairs" if step["batched"] else "single")
    if op == "prefetch_mask": return "prefetch_mask:+%d" % step["ahead"]
    if op == "encode_png_async": return "encode_png_async:" + ("wait" if step["wait"] else "nowait")
    if op in ("set_host_ordered", "set_single_image_size", "set_image_net"): return op + (":on" if step["on"] else ":off")
    if op == "set_long_term": return "set_long_term:" + step["variant"]
    return None


# ================================================================================================================== the state machine
def simulate(script, scaled_allowed=True, colors_allowed=True):
    """-> per step (variant | None, [hazards], expected long_term_available after it); ScriptError where a step leaves what fav.h allows"""
    st = dict(has_state=False, host=False, pref=[None] * NPREF, pref_next=0, lt=(), ring=[], pushes=0, scaled=False, img=False,
              last_scaled=False, inflight=False, last_hit=None, stylised=0, frameless_only=False)
    out = []

    def need(cond, i, what):
        if not cond:
            raise ScriptError("step %d (%s): %s" % (i, script[i]["op"], what))

    def avail(with_frames=False):
        m = 0
        while m < len(st["lt"]) and st["lt"][m] <= len(st["ring"]) and (not with_frames or st["ring"][-st["lt"][m]]):
            m += 1
        return m

    def push(has_frame):
        if st["lt"]:
            st["ring"].append(has_frame); st["pushes"] += 1
            del st["ring"][:-st["lt"][-1]]

    for i, step in enumerate(script):
        op, hz = step["op"], []
        var = variant_of(step, st)
        valid = [p for p in st["pref"] if p]
        if op in STYLISING:
            need(step["frame"] == st["stylised"], i, "the clip's frames are stylised in order")
            if i and script[i - 1]["op"] in REFUSED and i >= 2 and script[i - 2]["op"] in STYLISING:
                out[i - 1][1].append("refused-between-stylising")
        if op in STYLISING or op == "set_state":
            if st["inflight"]:
                hz.append("async-pending@" + ("set_state" if op == "set_state" else "first_frame" if op == "first_frame" else
                                              "long-term" if op.endswith("_lt") else "next_frame"))
            st["inflight"] = False
        if op == "first_frame":
            if valid: hz.append("lookahead-across-first_frame")
            if st["scaled"]: hz.append("scaled-first-then-last_input")
            st["last_scaled"] = st["scaled"]
            st["ring"] = []; st["pushes"] = 0; push(True); st["has_state"] = True; st["frameless_only"] = False
        elif op in ("next_frame_cert", "next_frame_flow", "next_frame_estimate"):
            need(st["has_state"], i, "no previous stylised frame")
            if op == "next_frame_estimate":
                need(step["frame"] >= 1, i, "no previous frame to estimate from")
            if op == "next_frame_flow":
                hit = [k for k, p in enumerate(st["pref"]) if p and p["frame"] == step["frame"] and p["structure"] == step["structure"]]
                if hit:
                    mode = st["pref"][hit[0]]["mode"]
                    need(mode == ("host" if st["host"] else "event"), i, "a slot of the other mode is valid")
                    st["pref"][hit[0]] = None
                    if mode == "host" and st["last_hit"] == "event": hz.append("host-hit-after-event-hit")
                    st["last_hit"] = mode
                    step["hit"] = True
                else:
                    step["hit"] = False
                    st["last_hit"] = None
                    if any(p["frame"] == step["frame"] for p in valid): hz.append("lookahead-miss")
            st["last_scaled"] = False; push(True); st["frameless_only"] = False
        elif op in ("next_frame_flows_lt", "next_frame_estimate_lt"):
            need(st["lt"], i, "long-term priors are off")
            need(st["has_state"], i, "no previous stylised frame")
            need(not valid, i, "a look-ahead is pending (fav_long_term.h: FAV_EINVAL)")
            if op == "next_frame_flows_lt":
                need(1 <= step["m"] <= avail(), i, "m = %d, the history serves %d" % (step["m"], avail()))
                if st["frameless_only"]:
                    need(st["ring"] == [False] and avail() == 1, i, "the history after set_state is one entry without a frame")
                    hz.append("set_state-then-lt-one-frameless-entry")
            else:
                need(avail(True) >= 1, i, "the history holds no previous frame")
            if st["pushes"] + 1 == st["lt"][-1] + 1: hz.append("history-ring-wraps")
            st["last_scaled"] = False; push(True); st["frameless_only"] = False
        elif op == "prefetch_mask":
            need(step["frame"] >= max(st["stylised"], 1), i, "a look-ahead is for a frame yet to come")
            need(step["ahead"] == step["frame"] - st["stylised"] + 1 and step["ahead"] in (1, 2), i, "one or two frames ahead")
            need(bool(step["sync"]) == st["host"], i, "host-ordered: the caller synchronises before the look-ahead (fav.h), and only then")
            need(not any(p["frame"] == step["frame"] and p["structure"] == step["structure"] for p in valid), i, "two look-aheads of one key")
            old = st["pref"][st["pref_next"]]
            if old: hz.append("unconsumed-lookahead-slot-reused")
            st["pref"][st["pref_next"]] = dict(frame=step["frame"], structure=step["structure"], mode="host" if st["host"] else "event")
            st["pref_next"] = (st["pref_next"] + 1) % NPREF
        elif op in ENCODING:
            need(st["has_state"], i, "no stylised frame yet")
            need(op not in COLORS_ONLY or colors_allowed, i, "the _colors encodes need Ho x Wo == H x W")
            if op in COLORS_ONLY: need(0 <= step["frame"] < st["stylised"], i, "the colours of a frame the clip has shown")
            if op == "encode_png_async": st["inflight"] = not step["wait"]
            elif op in ("encode_png", "encode_png_colors"): st["inflight"] = False      # (they wait for the asynchronous encodes)
        elif op == "set_state":
            need(0 <= step["source"] < st["stylised"], i, "the state of a frame not yet stylised")
            if valid: hz.append("lookahead-across-set_state")
            st["has_state"] = True; st["ring"] = []; st["pushes"] = 0; push(False); st["frameless_only"] = bool(st["lt"])
        elif op == "set_host_ordered":
            need(step["sync"], i, "fav.h: the mode is switched with the caller's queue drained")
            need(step["on"] != st["host"], i, "the mode is toggled")
            st["host"] = step["on"]; st["pref"] = [None] * NPREF
        elif op == "set_long_term":
            d = tuple(step["dists"])
            need(len(d) <= 4 and all(1 <= x <= 16 for x in d) and (not d or d[0] == 1) and all(a < b for a, b in zip(d, d[1:])), i, "bad distances")
            need({"on": not st["lt"] and d, "changed": st["lt"] and d and d != st["lt"], "off": st["lt"] and not d}[step["variant"]], i,
                 "not what its variant says")
            st["lt"] = d; st["ring"] = []; st["pushes"] = 0; st["frameless_only"] = False
            if d and st["has_state"]: push(False)
        elif op == "set_single_image_size":
            need(scaled_allowed, i, "the scaled path needs Ho x Wo == H x W")
            need(step["on"] != st["scaled"], i, "the mode is toggled")
            st["scaled"] = step["on"]
        elif op == "set_image_net":
            need(step["on"] != st["img"], i, "the mode is toggled")
            st["img"] = step["on"]
        elif op in ("refuse_flow_option", "refuse_small_workspace"):
            need(st["has_state"] and step["frame"] == st["stylised"] and step["frame"] >= 1, i, "the refusal must be the option's / the workspace's")
        elif op == "refuse_lt_distances":
            need(st["lt"] and st["has_state"] and not valid and step["frame"] == st["stylised"], i, "the refusal must be the count's")
            need(step["m"] > avail() and step["m"] <= 4, i, "m = %d is served (%d available)" % (step["m"], avail()))
        else:
            raise ScriptError("step %d: unknown op %r" % (i, op))
        if op in STYLISING: st["stylised"] += 1
        out.append((var, hz, avail() if st["lt"] else 0))
    return out


def annotate(script, scaled_allowed=True, colors_allowed=True):
    """write each step's tag: index, op, variant, arguments that matter, and the hazards simulate() finds in it"""
    for i, (step, (var, hz, _)) in enumerate(zip(script, simulate(script, scaled_allowed, colors_allowed))):
        args = " ".join("%s=%s" % (k, step[k]) for k in ("frame", "structure", "m", "source", "dists") if k in step)
        step["variant"] = var if step["op"] != "set_long_term" else step["variant"]
        step["tag"] = ("%s %s" % (var or step["op"], args)).strip() + "".join(" !" + h for h in hz)
    return script


def hazards_of(step):
    return [w[1:] for w in step["tag"].split() if w.startswith("!")]


# ================================================================================================================== the runner (GPU)
def make_clip(h, w, n, seed):
    """the clip of the pipeline tests (_clip of tests/test_gpu_parity.py: fav_amd.synth's smooth frames and flows)"""
    tests = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if tests not in sys.path:
        sys.path.insert(0, tests)
    from test_gpu_parity import _clip
    return _clip(h, w, n, seed)


def far_flows(h, w, i, d, seed):
    """the flows between frame i and frame i - d of a long-term step (d > 1)"""
    from fav_amd import synth
    bw = synth.backward_flow(h, w, seed + 1000 + 17 * i + d, std=2.0 + d)
    return bw, synth.forward_flow_from_backward(bw, seed + 2000 + 17 * i + d)


def bits_equal(a, b):
    import torch
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


class Mismatch(AssertionError):
    pass


class Runner:
    """one subject Stream through one script; every stylising step against a twin without history, every encode against a fresh Stream"""

    def __init__(self, favlib, net, img_net, name, script, device):
        import torch
        self.torch, self.fav, self.net, self.img_net, self.dev = torch, favlib, net, img_net, device
        self.name, self.cfg, self.script = name, SCRIPTS[name], script
        self.H, self.W = self.cfg["size"]
        o = dict(self.cfg["opts"])
        if "border" in o:
            o["border"] = favlib.BORDER_CPU if o["border"] == "cpu" else favlib.BORDER_STN
        self.opts = o
        self.shadowed = bool(o.get("fill_random"))
        n = 1 + max(s["frame"] for s in script if "frame" in s)
        frames, bws, fws = make_clip(self.H, self.W, n + 1, 100 * self.cfg["seed"])
        self.np_flows = {(i, 1): (bws[i], fws[i]) for i in range(1, n + 1)}
        self.frames = [self.T(f) for f in frames]
        self.flows = {}
        self.certs = {}
        self.stats = dict(steps=len(script), twins=0, bytes=0, values=0)

    def T(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def flow(self, i, d=1):
        """the device tensors the SUBJECT is given for (frame i, distance d): one pair per key, so that pointers repeat"""
        if (i, d) not in self.flows:
            if (i, d) not in self.np_flows:
                self.np_flows[(i, d)] = far_flows(self.H, self.W, i, d, 100 * self.cfg["seed"])
            self.flows[(i, d)] = tuple(self.T(x) for x in self.np_flows[(i, d)])
        return self.flows[(i, d)]

    def cert(self, i):
        if i not in self.certs:
            self.certs[i] = self.fav.consistency(*self.flow(i))
        return self.certs[i]

    def stream(self):
        self.stats["twins"] += 1
        return self.fav.Stream(self.net, self.H, self.W, **self.opts)

    def fail(self, i, what):
        raise Mismatch("script %s (seed %d), step %d [%s]: %s" % (self.name, self.cfg["seed"], i, self.script[i]["tag"], what))

    def same(self, i, what, a, b):
        if isinstance(a, int) or isinstance(b, int):
            if a != b: self.fail(i, "%s: %r, the twin's %r" % (what, a, b))
            return
        self.stats["values"] += 1; self.stats["bytes"] += a.numel() * a.element_size()
        if not bits_equal(a, b):
            t = self.torch
            n = int((a.contiguous().view(-1).view(t.uint8) != b.contiguous().view(-1).view(t.uint8)).sum()) if a.shape == b.shape else -1
            self.fail(i, "%s differs from the twin's (%d of %d bytes)" % (what, n, a.numel() * a.element_size()))

    # ---- one stylising call on a stream; c: how a device tensor is handed over (the twin gets copies at other addresses)
    def stylise(self, st, step, c):
        op, fr = step["op"], self.frames[step["frame"]]
        if op == "first_frame":
            return st.first_frame(c(fr), want_u8=True) + ([], [])
        if op == "next_frame_cert":
            return st.next_frame_cert(c(fr), c(self.flow(step["frame"])[0]), c(self.cert(step["frame"])), want_u8=True) + ([], [])
        if op == "next_frame_flow":
            bw, fw = self.flow(step["frame"])
            return st.next_frame_flow(c(fr), c(bw), c(fw), use_structure=step["structure"], want_u8=True) + ([], [])
        if op == "next_frame_estimate":
            f, u, bw, fw = st.next_frame_estimate(c(fr), c(self.frames[step.get("prev_frame", step["frame"] - 1)]), use_structure=step["structure"], want_u8=True,
                                                  batched=step["batched"], **FLOW_OPTS)
            return f, u, [bw], [fw]
        if op == "next_frame_flows_lt":
            d = self.lt[:step["m"]]
            return st.next_frame_flows_lt(c(fr), [c(self.flow(step["frame"], k)[0]) for k in d], [c(self.flow(step["frame"], k)[1]) for k in d],
                                          use_structure=step["structure"], want_u8=True) + ([], [])
        if op == "next_frame_estimate_lt":
            m = self.available(True)
            f, u, bws, fws = st.next_frame_estimate_lt(c(fr), use_structure=step["structure"], want_u8=True, **FLOW_OPTS)
            return f, u, [x.clone() for x in bws[:m]], [x.clone() for x in fws[:m]]
        raise ScriptError(op)

    def available(self, with_frames=False):
        m = 0
        while m < len(self.lt) and self.lt[m] <= len(self.ring) and (not with_frames or self.ring[-self.lt[m]][1] is not None):
            m += 1
        return m

    def push(self, state, frame):
        if self.lt:
            self.ring.append((state, frame))
            del self.ring[:-self.lt[-1]]

    def views(self, st, scaled):
        """state, last_input, last_padded_input (None, None after a frame at the scaled size: both views must refuse)"""
        if not scaled:
            return st.state(), st.last_input(), st.last_padded_input()
        for view in (st.last_input, st.last_padded_input):
            try:
                view()
            except self.fav.FavError:
                continue
            raise Mismatch("last_input() after a frame at the scaled size was not refused")
        return st.state(), None, None

    def compare(self, i, got, want, mask, scaled):
        names = ("f32 frame", "u8 frame", "state()", "last_input()", "last_padded_input()")
        for name, a, b in zip(names, got, want):
            if a is not None or b is not None:
                self.same(i, name, a, b)
        if mask is not None:
            self.same(i, "last_mask()", *mask)

    def long_term_twin(self, i, step, sub_flows):
        """favlib.long_term_input + Net.forward on what the runner recorded itself: the states (and frames) of the distances served, their
        flows, and each distance's certainty from a fresh Stream's plain 1-distance call"""
        t, fav = self.torch, self.fav
        fr = self.frames[step["frame"]]
        if step["op"] == "next_frame_flows_lt":
            d = self.lt[:step["m"]]
            fl = [self.flow(step["frame"], k) for k in d]
            bws, fws = [f[0].clone() for f in fl], [f[1].clone() for f in fl]
        else:
            d = self.lt[:self.available(True)]
            bws, fws = fav.flow_pairs([self.frames[self.ring[-k][1]].clone() for k in d], [fr.clone() for _ in d], FLOW_OPTS)
            for k in range(len(d)):
                self.same(i, "backward flow of distance %d" % d[k], sub_flows[0][k], bws[k])
                self.same(i, "forward flow of distance %d" % d[k], sub_flows[1][k], fws[k])
        states = [self.ring[-k][0].clone() for k in d]
        certs, mask = [], None
        for k in range(len(d)):
            tw = self.stream()
            tw.set_state(states[k])
            tw.next_frame_flow(fr.clone(), bws[k], fws[k], use_structure=step["structure"])
            certs.append(tw.last_input()[6].contiguous())
            if k == 0: mask = tw.last_mask()
            tw.close()
        p = self.net.input_pad()
        padded, _ = fav.long_term_input(fr.clone(), states, bws, certs, border=self.opts.get("border", fav.BORDER_STN), pad=p)
        in7 = padded[p:p + self.H, p:p + self.W, :7].permute(2, 0, 1).contiguous()
        # The frame itself is not composed here.  Net.forward returns 150 tanh in BGR; the stream's frames are de-processed by the last
        # layer's own epilogue, rgb = (150 tanh + mean) / 255 (the kernels are compiled with contraction on: presumably one fma of product
        # and sum), which arithmetic on the ROUNDED product does not restate bit for bit (measured on the MI355X, one distance, the same
        # padded input: (Net.forward + mean) / 255 differs from the subject's frame in 7528 of 41472 bytes, while a fresh Stream's frame
        # is equal).  A step that uses ONE distance is held, frame included, by a
        # Stream twin (run()); with more distances the composition holds the input -- where the history enters -- and the frame is held
        # to its own views: state() and the quantised bytes
        return (None, None, None, in7, padded), mask

    def quantised(self, f):
        """image.save's quantisation (fav.h): clamp to [0, 1], x 255, truncate -> [Ho][Wo][3]"""
        return (f.clamp(0, 1) * 255).to(self.torch.uint8).permute(1, 2, 0).contiguous()

    # ---- encodes
    def encode(self, st, step, c, asynchronous=False):
        """-> (buffer, byte count tensor | None) of one encoding call, enqueued"""
        fav, t, op = self.fav, self.torch, step["op"]
        if op in ("encode_png", "encode_png_async", "encode_png_colors"):
            out, n = st.png_buffers()
            out.zero_()
            if op == "encode_png_colors": st.encode_png_colors_into(c(self.frames[step["frame"]]), step["matrix"], out, n)
            elif asynchronous: st.encode_png_async_into(out, n)
            else: st.encode_png_into(out, n)
            return out, n
        if op == "encode_yuv_layout":
            lay = fav.yuv_layout(chroma=fav.YUV_420, matrix=step["matrix"], depth=step["depth"])
            out = t.zeros(fav.yuv_layout_frame_bytes(st.Wo, st.Ho, lay), dtype=t.uint8, device=self.dev)
            st.encode_yuv_layout_into(out, lay)
            return out, None
        fmt = fav.yuv_format(chroma=step["chroma"], matrix=step["matrix"], full_range=step["full_range"])
        out = t.zeros(fav.yuv_frame_bytes(st.Wo, st.Ho, fmt), dtype=t.uint8, device=self.dev)
        if op == "encode_yuv_colors": st.encode_yuv_colors_into(c(self.frames[step["frame"]]), out, fmt)
        else: st.encode_yuv_into(out, fmt)
        return out, None

    def check_encode(self, i, step, got, state):
        """the subject's bytes against the same encode of a fresh Stream that holds `state`"""
        tw = self.stream()
        tw.set_state(state)
        want = self.encode(tw, step, lambda x: x.clone())
        self.torch.cuda.synchronize()
        if got[1] is not None:
            n, m = int(got[1].item()), int(want[1].item())
            if n != m or n <= 0: self.fail(i, "the file is %d bytes, the fresh stream's %d" % (n, m))
            self.same(i, "the file's bytes", got[0][:n], want[0][:n])
        else:
            self.same(i, "the planes' bytes", got[0], want[0])
        tw.close()

    def refused(self, i, step):
        fav, t, sub = self.fav, self.torch, self.subject
        fr = self.frames[step["frame"]]
        try:
            if step["op"] == "refuse_lt_distances":
                fl = [self.flow(step["frame"], k + 1) for k in range(step["m"])]
                sub.next_frame_flows_lt(fr, [f[0] for f in fl], [f[1] for f in fl])
            else:
                bad = step["op"] == "refuse_flow_option"
                estimate_raw(fav, sub, fr, self.frames[step["frame"] - 1], dict(FLOW_OPTS, median=4) if bad else FLOW_OPTS, 0 if bad else -256)
        except fav.FavError:
            return
        self.fail(i, "the call was not refused")

    # ---- the script
    def run(self):
        t, fav = self.torch, self.fav
        self.subject = sub = self.stream()
        shadow = self.stream() if self.shadowed else None
        self.lt, self.ring = (), []
        recorded, scaled, img, host, deferred = [], False, False, False, None
        ident, copy = (lambda x: x), (lambda x: x.clone())
        expect = simulate(self.script, self.cfg["scaled"], self.cfg["colors"])
        for i, step in enumerate(self.script):
            op = step["op"]
            if op in STYLISING:
                prev = sub.state() if recorded else None
                got = self.stylise(sub, step, ident)
                was_scaled = op == "first_frame" and scaled
                mask = None
                if shadow is not None:
                    want = self.stylise(shadow, step, copy)
                    tw = shadow
                elif op.endswith("_lt"):
                    want5, m = self.long_term_twin(i, step, got[2:])
                    self.compare(i, (None, None, None) + self.views(sub, False)[1:], want5, (sub.last_mask(), m), False)
                    served = step["m"] if op == "next_frame_flows_lt" else self.available(True)
                    if served == 1:                                   # fav_long_term.h: with m = 1 the frame is next_frame_flow's, byte for byte
                        tw = self.stream()
                        tw.set_state(prev.clone())
                        plain = dict(step, op="next_frame_flow") if op == "next_frame_flows_lt" else dict(step, op="next_frame_estimate", batched=True)
                        if op == "next_frame_estimate_lt":
                            plain["prev_frame"] = self.ring[-1][1]
                        want = self.stylise(tw, plain, copy)
                    else:
                        tw = None
                        self.same(i, "state() against the returned frame", sub.state(), got[0])
                        self.same(i, "u8 frame against the quantised f32 frame", got[1], self.quantised(got[0]))
                else:
                    tw = self.stream()
                    if op == "first_frame":
                        if img: tw.set_image_net(self.img_net)
                        if scaled: tw.set_single_image_size(*SCALED_SIZE)
                    else:
                        tw.set_state(prev.clone())
                    want = self.stylise(tw, step, copy)
                if tw is not None:
                    want5 = want[:2] + self.views(tw, was_scaled)
                    if op != "first_frame": mask = (sub.last_mask(), tw.last_mask())      # (a frame without a prior has no mask)
                    for k, (a, b) in enumerate(zip(got[2] + got[3], want[2] + want[3])):
                        self.same(i, "estimated flow %d" % k, a, b)
                    if tw is not shadow: tw.close()
                    self.compare(i, got[:2] + self.views(sub, was_scaled), want5, mask, was_scaled)
                if op == "first_frame": self.ring = []
                self.push(got[0].clone(), step["frame"])
                recorded.append(got[0].clone())
                if self.lt:
                    self.same(i, "long_term_available()", sub.long_term_available(), self.available())
                    self.same(i, "long_term_available() (state machine)", sub.long_term_available(), expect[i][2])
                    if shadow is not None: self.same(i, "long_term_available() (twin)", sub.long_term_available(), shadow.long_term_available())
                if deferred is not None:                              # the asynchronous encode that ran next to this frame
                    sub.wait_png(); t.cuda.synchronize()
                    self.check_encode(*deferred); deferred = None
            elif op == "prefetch_mask":
                if step["sync"]: t.cuda.synchronize()
                sub.prefetch_mask(self.frames[step["frame"]], *self.flow(step["frame"]), use_structure=step["structure"])
            elif op in ENCODING:
                state = sub.state()
                if op == "encode_png_async":
                    got = self.encode(sub, step, ident, asynchronous=True)
                    if step["wait"]:
                        sub.wait_png(); t.cuda.synchronize()
                        self.check_encode(i, step, got, state)
                    else:
                        deferred = (i, step, got, state)              # nothing waits: the next frame runs next to the encoder
                else:
                    got = self.encode(sub, step, ident)
                    t.cuda.synchronize()
                    self.check_encode(i, step, got, state)
            elif op == "set_state":
                x = recorded[step["source"]]
                sub.set_state(x)
                if shadow is not None: shadow.set_state(x.clone())
                self.ring = []; self.push(x.clone(), None)
                if deferred is not None:                              # the encoder read the buffer set_state has just overwritten
                    sub.wait_png(); t.cuda.synchronize()
                    self.check_encode(*deferred); deferred = None
                self.same(i, "state() after set_state", sub.state(), x)
            elif op == "set_host_ordered":
                t.cuda.synchronize()
                sub.set_host_ordered(step["on"]); host = step["on"]
            elif op == "set_long_term":
                for s in (sub, shadow):
                    if s is not None: s.set_long_term(step["dists"])
                self.lt, self.ring = tuple(step["dists"]), []
                if recorded: self.push(sub.state(), None)
                self.same(i, "long_term_available() after set_long_term", sub.long_term_available(), self.available())
            elif op == "set_single_image_size":
                scaled = step["on"]
                for s in (sub, shadow):
                    if s is not None: s.set_single_image_size(*(SCALED_SIZE if scaled else (0, 0)))
            elif op == "set_image_net":
                img = step["on"]
                for s in (sub, shadow):
                    if s is not None: s.set_image_net(self.img_net if img else None)
            elif op in REFUSED:
                self.refused(i, step)
            else:
                raise ScriptError(op)
        if deferred is not None:
            sub.wait_png(); t.cuda.synchronize()
            self.check_encode(*deferred)
        t.cuda.synchronize()
        self.net.check()
        sub.close()
        if shadow is not None: shadow.close()
        return self.stats


def estimate_raw(favlib, st, frame, prev, flow_opts, bytes_off):
    """fav_stream_next_frame_estimate_ex3 itself (Stream.next_frame_estimate asks the workspace query first, which would refuse a bad
    option before the stream sees it).  bytes_off: added to the single-flow workspace size that is declared (the buffer has the full size)"""
    import ctypes as C
    import torch
    good = {k: v for k, v in flow_opts.items() if k != "median"}
    nb = favlib.flow_workspace_bytes(st.W, st.H, **good)
    ws = torch.empty(nb, dtype=torch.uint8, device=frame.device)
    bw = torch.empty((st.H, st.W, 2), dtype=torch.float32, device=frame.device); fw = torch.empty_like(bw)
    f = torch.empty((3, st.Ho, st.Wo), dtype=torch.float32, device=frame.device)
    o = favlib._flow_opts_ex3(flow_opts)
    favlib._check(favlib.lib().fav_stream_next_frame_estimate_ex3(st.h, favlib._p(frame), favlib._p(prev), C.byref(o), 0, favlib._p(bw), favlib._p(fw),
                                                                 favlib._p(ws), C.c_size_t(nb + bytes_off), favlib._p(f), None, favlib._stream()))
    return f
