"""ctypes binding of libfav (include/fav.h) -- thin plumbing for the tests and bench.py.

The product is the C-ABI shared library ``fast-artistic-videos_amd/libfav.so`` (hand-written HIP for
gfx950 + C++ host code).  This module only moves pointers: device buffers are torch CUDA(=HIP)
tensors, ``tensor.data_ptr()`` and the current torch stream are handed to the C entry points.  There
is NO Python/CPU fallback: if the library is missing, or no HIP device is present, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # fast-artistic-videos_amd/
# FAV_AMD_LIB: another build of the library for THIS binding (tests / A-B scripts load libfav_diag.so, the build whose kernel-selection
# switches are live; the release library reads none of them)
LIB_PATH = os.environ.get("FAV_AMD_LIB") or os.path.join(_PKG, "libfav.so")
DIAG_LIB_PATH = os.path.join(_PKG, "libfav_diag.so")
BORDER_STN, BORDER_CPU = 0, 1

_lib = None


class FavError(RuntimeError):
    pass


def build(verbose: bool = False) -> None:
    """Compile libfav.so and the drop-in executables for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess
    subprocess.check_call(["make", "-C", _PKG, "-j8", "all"], stdout=None if verbose else subprocess.DEVNULL)


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FavError(f"{LIB_PATH} is missing: build it with `make -C {_PKG}` "
                       "(python -c 'import __graft_entry__ as g; g.build()'); there is no fallback path")
    L = C.CDLL(LIB_PATH)
    L.fav_last_error.restype = C.c_char_p
    L.fav_consistency_workspace_bytes.restype = C.c_size_t
    L.fav_consistency_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.fav_net_param_count.restype = C.c_longlong
    L.fav_net_param_count.argtypes = [C.c_void_p]
    L.fav_stream_last_mask.restype = C.c_void_p
    L.fav_stream_last_mask.argtypes = [C.c_void_p]
    L.fav_net_destroy.argtypes = [C.c_void_p]; L.fav_net_destroy.restype = None
    L.fav_stream_destroy.argtypes = [C.c_void_p]; L.fav_stream_destroy.restype = None
    L.fav_free_host.argtypes = [C.c_void_p]; L.fav_free_host.restype = None
    for f in (L.fav_png_capacity, L.fav_png_workspace_bytes):
        f.restype = C.c_size_t; f.argtypes = [C.c_int, C.c_int]
    L.fav_vr_destroy.argtypes = [C.c_void_p]; L.fav_vr_destroy.restype = None
    L.fav_vr_last_mask.restype = C.c_void_p
    L.fav_vr_last_mask.argtypes = [C.c_void_p]
    L.fav_png_crc32_combine_host.restype = C.c_uint32; L.fav_png_crc32_combine_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.fav_flow_workspace_bytes.restype = C.c_size_t
    L.fav_flow_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.fav_flow_pairs_workspace_bytes.restype = C.c_size_t
    L.fav_flow_pairs_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.fav_flow_workspace_bytes_ex.restype = C.c_size_t
    L.fav_flow_workspace_bytes_ex.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.fav_flow_pairs_workspace_bytes_ex.restype = C.c_size_t
    L.fav_flow_pairs_workspace_bytes_ex.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.fav_flow_workspace_bytes_ex2.restype = C.c_size_t
    L.fav_flow_workspace_bytes_ex2.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.fav_flow_pairs_workspace_bytes_ex2.restype = C.c_size_t
    L.fav_flow_pairs_workspace_bytes_ex2.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.fav_flow_workspace_bytes_ex3.restype = C.c_size_t
    L.fav_flow_workspace_bytes_ex3.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.fav_flow_pairs_workspace_bytes_ex3.restype = C.c_size_t
    L.fav_flow_pairs_workspace_bytes_ex3.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.fav_yuv_frame_bytes.restype = C.c_size_t
    L.fav_yuv_frame_bytes.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.fav_yuv_layout_frame_bytes.restype = C.c_size_t
    L.fav_yuv_layout_frame_bytes.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.fav_scene_change_workspace_bytes.restype = C.c_size_t
    L.fav_scene_change_workspace_bytes.argtypes = []
    L.fav_stream_long_term_workspace_bytes.restype = C.c_size_t
    L.fav_stream_long_term_workspace_bytes.argtypes = [C.c_void_p, C.c_void_p]
    L.fav_stream_long_term_available.restype = C.c_int
    L.fav_stream_long_term_available.argtypes = [C.c_void_p]
    L.fav_stream_set_long_term.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.fav_long_term_input_f32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fav_stream_next_frame_flows_lt.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fav_stream_next_frame_estimate_lt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fav_vr_set_f32.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.fav_vr_get_padded_input_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


EXPORTS = [
    "fav_last_error", "fav_version", "fav_device_count", "fav_warp_bdhw_f32", "fav_consistency_workspace_bytes",
    "fav_consistency_u8", "fav_min_filter_f32", "fav_assemble_input_f32", "fav_net_create", "fav_net_pack_host",
    "fav_net_create_from_blob", "fav_net_destroy", "fav_net_describe_host", "fav_t7_describe_host", "fav_net_param_count",
    "fav_net_output_size", "fav_net_forward", "fav_net_profile_enable", "fav_net_profile_read_host",
    "fav_conv2d_nchw_f32", "fav_conv_transpose2d_nchw_f32", "fav_stream_create", "fav_stream_destroy",
    "fav_stream_set_image_net", "fav_stream_first_frame", "fav_stream_next_frame_cert", "fav_stream_next_frame_flow", "fav_stream_prefetch_mask",
    "fav_stream_get_state",
    "fav_stream_set_state", "fav_stream_last_mask", "fav_stream_get_input_f32", "fav_stream_get_padded_input_f32", "fav_stream_output_size", "fav_stream_set_host_ordered",
    "fav_png_capacity", "fav_png_workspace_bytes", "fav_png_encode_rgb8", "fav_png_encode_f32", "fav_stream_encode_png", "fav_stream_encode_png_async", "fav_stream_wait_png", "fav_png_tables_host", "fav_png_crc32_combine_host", "fav_read_flo_host", "fav_read_pnm_host", "fav_write_pgm_host",
    "fav_write_png_rgb8_host", "fav_free_host",
    "fav_vr_create", "fav_vr_destroy", "fav_vr_face", "fav_vr_finish_frame", "fav_vr_output_sizes", "fav_vr_get_f32",
    "fav_vr_map_host", "fav_temporal_loss_host", "fav_sequential_sum_f32", "fav_read_flo_into_host", "fav_read_pnm_into_host", "fav_net_set_precision", "fav_net_check", "fav_net_set_shared_device", "fav_net_forget_stream",
    "fav_scale_bicubic_f32", "fav_stream_set_single_image_size",
    "fav_vr_face_flow", "fav_vr_prefetch_mask", "fav_vr_last_mask",
    "fav_flow_workspace_bytes", "fav_flow_rgb8", "fav_flow_grey_f32", "fav_flow_down_f32", "fav_flow_up_f32", "fav_flow_coefficients_f32",
    "fav_flow_sweeps_f32", "fav_stream_next_frame_estimate",
    "fav_flow_pairs_workspace_bytes", "fav_flow_pairs_rgb8",
    "fav_flow_coefficients_robust_f32", "fav_flow_sweeps_robust_f32",
    "fav_flow_workspace_bytes_ex", "fav_flow_rgb8_ex", "fav_flow_pairs_workspace_bytes_ex", "fav_flow_pairs_rgb8_ex",
    "fav_stream_next_frame_estimate_ex", "fav_flow_coefficients_grad_f32", "fav_flow_sweeps_grad_f32",
    "fav_flow_workspace_bytes_ex2", "fav_flow_rgb8_ex2", "fav_flow_pairs_workspace_bytes_ex2", "fav_flow_pairs_rgb8_ex2",
    "fav_stream_next_frame_estimate_ex2", "fav_flow_match_f32", "fav_flow_match_check", "fav_flow_coefficients_prior_f32",
    "fav_flow_workspace_bytes_ex3", "fav_flow_rgb8_ex3", "fav_flow_pairs_workspace_bytes_ex3", "fav_flow_pairs_rgb8_ex3",
    "fav_stream_next_frame_estimate_ex3", "fav_flow_median_f32",
    "fav_vr_equi_to_faces_rgb8",
    "fav_yuv_frame_bytes", "fav_yuv_to_rgb8", "fav_rgb8_to_yuv", "fav_rgb_f32_to_yuv", "fav_stream_encode_yuv",
    "fav_y4m_parse_header_host", "fav_y4m_format_header_host",
    "fav_scene_change_workspace_bytes", "fav_scene_change_rgb8",
    "fav_color_transfer_rgb8", "fav_color_transfer_yuv", "fav_stream_encode_png_colors", "fav_stream_encode_yuv_colors",
    "fav_structure_f32",
]
# include/fav_yuv.h: 4:2:2 and 9- to 16-bit Y4M frames
EXPORTS_YUV = [
    "fav_yuv_layout_frame_bytes", "fav_yuv_layout_to_rgb8", "fav_rgb8_to_yuv_layout", "fav_rgb_f32_to_yuv_layout",
    "fav_stream_encode_yuv_layout", "fav_y4m_parse_stream_header_host", "fav_y4m_format_stream_header_host",
]


# include/fav_long_term.h: long-term priors
EXPORTS_LONG_TERM = [
    "fav_long_term_input_f32", "fav_stream_set_long_term", "fav_stream_long_term_available", "fav_stream_next_frame_flows_lt",
    "fav_stream_long_term_workspace_bytes", "fav_stream_next_frame_estimate_lt",
]
# include/fav_vr_state.h: writing a VR object's faces
EXPORTS_VR_STATE = ["fav_vr_set_f32", "fav_vr_get_padded_input_f32"]


def _check(rc: int) -> None:
    if rc != 0:
        raise FavError(f"libfav error {rc}: {lib().fav_last_error().decode(errors='replace')}")


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise FavError("no HIP device visible to torch: libfav has no CPU fallback")
    return torch


def _p(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream() -> C.c_void_p:
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _chk_f32(t, name):
    torch = _torch()
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise FavError(f"{name} must be a contiguous float32 CUDA tensor")   # BilinearSamplerBDHW.lua:26-42


def device_count() -> int:
    n = lib().fav_device_count()
    if n < 0:
        _check(n)
    return n


# ------------------------------------------------------------------------------------------------ ops
def warp(img, flow, border: int = BORDER_STN):
    """nn.BilinearSamplerBDHW():forward({img, flow}) (stnbdhw/BilinearSamplerBDHW.lua:54-82): 3-D inputs get a
    batch dimension added and removed."""
    torch = _torch(); _chk_f32(img, "img"); _chk_f32(flow, "flow")
    squeeze = img.dim() == 3
    if squeeze:
        img, flow = img[None], flow[None]
    b, c, h, w = img.shape
    assert flow.shape[0] == b and flow.shape[1] == 2
    ho, wo = flow.shape[2], flow.shape[3]
    out = torch.empty((b, c, ho, wo), dtype=torch.float32, device=img.device)
    _check(lib().fav_warp_bdhw_f32(_p(img), _p(flow), _p(out), b, c, h, w, ho, wo, border, _stream()))
    return out[0] if squeeze else out


def consistency(flow1_flo, flow2_flo, rgb_hwc=None):
    """consistencyChecker flow1.flo flow2.flo out.pgm [img.ppm]: inputs are the .flo payloads [H][W][2]."""
    torch = _torch(); _chk_f32(flow1_flo, "flow1"); _chk_f32(flow2_flo, "flow2")
    h, w, _ = flow1_flo.shape
    out = torch.empty((h, w), dtype=torch.uint8, device=flow1_flo.device)
    ws_bytes = lib().fav_consistency_workspace_bytes(w, h, 1 if rgb_hwc is not None else 0)
    ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=flow1_flo.device)
    _check(lib().fav_consistency_u8(_p(flow1_flo), _p(flow2_flo), _p(rgb_hwc), _p(out), w, h, _p(ws),
                                    C.c_size_t(ws_bytes), _stream()))
    return out


STRUCTURE_WIDE, STRUCTURE_PACKED = 0, 1


def structure(rgb_hwc, pack_cus: int = 0, q0: int = 0, ws=None, out=None, avg=None):
    """fav_structure_f32: the structure map of the 4-argument check of a u8 [H][W][3] frame -> (map [H][W] f32, avg [1] f32, form_ran).
    pack_cus = 0: the wide launch form (what consistency() runs); 1..4: the packed form of the look-ahead path, q0 (0..7) its placement
    word.  form_ran: STRUCTURE_WIDE | STRUCTURE_PACKED, the form that was launched.  ws / out / avg: the caller's workspace (u8, at least
    fav_consistency_workspace_bytes(W, H, 1) elements) and output tensors (tests hand them in pre-filled)."""
    torch = _torch()
    if not (rgb_hwc.is_cuda and rgb_hwc.dtype == torch.uint8 and rgb_hwc.dim() == 3 and rgb_hwc.shape[2] == 3 and rgb_hwc.is_contiguous()):
        raise FavError("structure: the frame must be a contiguous uint8 CUDA tensor [H][W][3]")
    h, w = rgb_hwc.shape[0], rgb_hwc.shape[1]
    if ws is None:
        ws = torch.empty((max(lib().fav_consistency_workspace_bytes(w, h, 1), 1),), dtype=torch.uint8, device=rgb_hwc.device)
    if out is None:
        out = torch.empty((h, w), dtype=torch.float32, device=rgb_hwc.device)
    if avg is None:
        avg = torch.empty(1, dtype=torch.float32, device=rgb_hwc.device)
    _chk_f32(out, "out"); _chk_f32(avg, "avg")
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and out.numel() >= h * w
    form = C.c_int(-1)
    _check(lib().fav_structure_f32(_p(rgb_hwc), w, h, _p(ws), C.c_size_t(ws.numel()), _p(out), _p(avg), int(pack_cus), int(q0),
                                   C.byref(form), _stream()))
    return out, avg, form.value


def min_filter(cert, r: int = 7):
    torch = _torch(); _chk_f32(cert, "cert")
    out = torch.empty_like(cert)
    _check(lib().fav_min_filter_f32(_p(cert), _p(out), cert.shape[-2], cert.shape[-1], r, _stream()))
    return out


def assemble(frame_rgb, warped_rgb=None, cert=None):
    torch = _torch(); _chk_f32(frame_rgb, "frame")
    _, h, w = frame_rgb.shape
    out = torch.empty((7, h, w), dtype=torch.float32, device=frame_rgb.device)
    _check(lib().fav_assemble_input_f32(_p(frame_rgb), _p(warped_rgb), _p(cert), _p(out), h, w, _stream()))
    return out


LONG_TERM_MAX, LONG_TERM_MAX_DISTANCE = 4, 16


def _ptr_array(ts):
    """a HOST array of device pointers, one per tensor"""
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def long_term_input(frame_u8_hwc, states, backward_flos, certs, border: int = BORDER_STN, pad: int = 0, fill_random: bool = False,
                    seed: int = 0, index: int = 0, want_cert: bool = True):
    """fav_long_term_input_f32: the network input of a frame from K = len(states) priors in ascending distance (states [3][Hs][Ws],
    backward_flos [H][W][2], certs [H][W] eroded certainty) -> (padded input [H + 2 pad][W + 2 pad][8], merged certainty [H][W] | None)"""
    torch = _torch()
    h, w = frame_u8_hwc.shape[0], frame_u8_hwc.shape[1]
    for t in list(states) + list(backward_flos) + list(certs):
        _chk_f32(t, "long_term_input: every state, flow and certainty")
    if not (len(states) == len(backward_flos) == len(certs)) or any(t.shape != states[0].shape for t in states) or \
            any(tuple(t.shape) != (h, w, 2) for t in backward_flos) or any(tuple(t.shape) != (h, w) for t in certs):
        raise FavError("long_term_input: K states of one size, K flows [H][W][2] and K certainties [H][W]")
    hs, ws = (states[0].shape[1], states[0].shape[2]) if states else (0, 0)
    out = torch.empty((h + 2 * pad, w + 2 * pad, 8) if 0 <= pad else (0,), dtype=torch.float32, device=frame_u8_hwc.device)
    cert = torch.empty((h, w), dtype=torch.float32, device=frame_u8_hwc.device) if want_cert else None
    _check(lib().fav_long_term_input_f32(_p(frame_u8_hwc), len(states), _ptr_array(states), hs, ws, _ptr_array(backward_flos), _ptr_array(certs),
                                         border, h, w, pad, 1 if fill_random else 0, seed, index, _p(out), _p(cert), _stream()))
    return out, cert


def conv2d(x, weight, bias=None, stride=1, pad=0, gamma=None, beta=None, eps=1e-5, relu=False):
    torch = _torch(); _chk_f32(x, "x"); _chk_f32(weight, "weight")
    cin, h, w = x.shape; cout, _, k, _ = weight.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    out = torch.empty((cout, oh, ow), dtype=torch.float32, device=x.device)
    _check(lib().fav_conv2d_nchw_f32(_p(x), cin, h, w, _p(weight), _p(bias), cout, k, stride, pad, _p(gamma), _p(beta),
                                     C.c_float(eps), 1 if relu else 0, _p(out), _stream()))
    return out


def conv_transpose2d(x, weight, bias=None, stride=2, pad=0, adj=0, gamma=None, beta=None, eps=1e-5, relu=False):
    """nn.SpatialFullConvolution(cin, cout, k, k, stride, stride, pad, pad, adj, adj) [+ InstanceNormalization [+ ReLU]] of a [Cin][H][W]
    tensor; weight [Cin][Cout][k][k] (torch.nn.functional.conv_transpose2d's layout)."""
    torch = _torch(); _chk_f32(x, "x"); _chk_f32(weight, "weight")
    cin, h, w = x.shape; _, cout, k, _ = weight.shape
    oh, ow = (h - 1) * stride - 2 * pad + k + adj, (w - 1) * stride - 2 * pad + k + adj
    out = torch.empty((cout, oh, ow), dtype=torch.float32, device=x.device)
    _check(lib().fav_conv_transpose2d_nchw_f32(_p(x), cin, h, w, _p(weight), _p(bias), cout, k, stride, pad, adj, _p(gamma), _p(beta),
                                               C.c_float(eps), 1 if relu else 0, _p(out), _stream()))
    return out


def scale_bicubic(x, hd: int, wd: int):
    """image.scale(x, wd, hd, 'bicubic') [recalled] of a float [C][H][W] tensor: the resampling behind -scale_factor."""
    torch = _torch(); _chk_f32(x, "x")
    c, h, w = x.shape
    out = torch.empty((c, hd, wd), dtype=torch.float32, device=x.device)
    _check(lib().fav_scale_bicubic_f32(_p(x), _p(out), c, h, w, hd, wd, _stream()))
    return out


# ------------------------------------------------------------------------------------------------ optical flow
class _FlowOpts(C.Structure):
    _fields_ = [("levels", C.c_int), ("warps", C.c_int), ("iters", C.c_int), ("alpha", C.c_float), ("sweeps_per_launch", C.c_int),
                ("smooth_eps", C.c_float)]


class _FlowOptsEx(C.Structure):
    _fields_ = [("base", _FlowOpts), ("data_term", C.c_int)]


FLOW_DATA_BRIGHTNESS, FLOW_DATA_GRADIENT = 0, 1
_DATA_KEYS = {"data_term", "gradient_data"}


def _flow_opts(opts) -> "_FlowOpts":
    unknown = set(opts) - {f for f, _ in _FlowOpts._fields_}
    if unknown:
        raise FavError(f"unknown flow option(s) {sorted(unknown)}")
    return _FlowOpts(int(opts.get("levels", 0)), int(opts.get("warps", 0)), int(opts.get("iters", 0)), float(opts.get("alpha", 0.0)),
                     int(opts.get("sweeps_per_launch", 0)), float(opts.get("smooth_eps", 0.0)))


def _flow_opts_ex(opts) -> "_FlowOptsEx":
    """fav_flow_opts_ex of the flow options: the fields of fav_flow_opts plus data_term= (0 | 1) or gradient_data= (bool), which select
    the data term; every Python entry goes through the _ex entries of the library"""
    if _DATA_KEYS <= set(opts) and int(opts["data_term"]) != (FLOW_DATA_GRADIENT if opts["gradient_data"] else FLOW_DATA_BRIGHTNESS):
        raise FavError("flow options: data_term and gradient_data contradict each other")
    term = int(opts["data_term"]) if "data_term" in opts else (FLOW_DATA_GRADIENT if opts.get("gradient_data") else FLOW_DATA_BRIGHTNESS)
    return _FlowOptsEx(_flow_opts({k: v for k, v in opts.items() if k not in _DATA_KEYS}), term)


class _FlowOptsEx2(C.Structure):
    _fields_ = [("ex", _FlowOptsEx), ("match_beta", C.c_float), ("match_radius", C.c_int)]


_MATCH_KEYS = {"match_beta", "match_radius"}


def _flow_opts_ex2(opts) -> "_FlowOptsEx2":
    """fav_flow_opts_ex2 of the flow options: those of _flow_opts_ex plus match_beta= (0 = off, negative = the default weight) and
    match_radius= (0 = default), the matching prior; every Python entry goes through the _ex2 entries of the library"""
    return _FlowOptsEx2(_flow_opts_ex({k: v for k, v in opts.items() if k not in _MATCH_KEYS}), float(opts.get("match_beta", 0.0)),
                        int(opts.get("match_radius", 0)))


class _FlowOptsEx3(C.Structure):
    _fields_ = [("ex2", _FlowOptsEx2), ("median", C.c_int)]


def _flow_opts_ex3(opts) -> "_FlowOptsEx3":
    """fav_flow_opts_ex3 of the flow options: those of _flow_opts_ex2 plus median= (0 = off, 3 or 5: the side of the window of the median
    filter behind every warp); every Python entry goes through the _ex3 entries of the library"""
    return _FlowOptsEx3(_flow_opts_ex2({k: v for k, v in opts.items() if k != "median"}), int(opts.get("median", 0)))


def flow_workspace_bytes(w: int, h: int, **opts) -> int:
    """fav_flow_workspace_bytes_ex3 (host only); raises on a bad size or option"""
    o = _flow_opts_ex3(opts)
    n = lib().fav_flow_workspace_bytes_ex3(w, h, C.cast(C.pointer(o), C.c_void_p))
    if n == 0:
        _check(-1)
    return n


def flow_rgb8(a, b, **opts):
    """fav_flow_rgb8: the flow w "from a to b", b(p + w(p)) ~ a(p), of two u8 [H][W][3] frames -> .flo payload [H][W][2] (u, v).
    opts: levels, warps, iters, alpha, sweeps_per_launch (0 / absent = default); smooth_eps > 0 turns the edge-preserving smoothness on;
    data_term=1 / gradient_data=True takes the data term on the image gradients (frames whose lighting changes); match_beta != 0 turns
    the block-matching prior on (negative: the default weight), match_radius is its search radius at half resolution; median=3 | 5
    replaces the flow by its 3 x 3 | 5 x 5 median after every warp."""
    torch = _torch()
    if not (a.is_cuda and b.is_cuda and a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.is_contiguous() and b.is_contiguous() and
            a.dim() == 3 and a.shape[2] == 3 and a.shape == b.shape):
        raise FavError("flow_rgb8: a and b must be contiguous uint8 CUDA tensors [H][W][3] of one size")
    h, w = a.shape[0], a.shape[1]
    o = _flow_opts_ex3(opts)
    nb = flow_workspace_bytes(w, h, **opts)
    ws = torch.empty(nb, dtype=torch.uint8, device=a.device)
    out = torch.empty((h, w, 2), dtype=torch.float32, device=a.device)
    _check(lib().fav_flow_rgb8_ex3(_p(a), _p(b), w, h, C.byref(o), _p(out), _p(ws), C.c_size_t(nb), _stream()))
    return out


FLOW_MAX_PAIRS = 8


def flow_pairs_workspace_bytes(w: int, h: int, n_pairs: int, **opts) -> int:
    """fav_flow_pairs_workspace_bytes_ex3 (host only); raises on a bad size, pair count or option"""
    o = _flow_opts_ex3(opts)
    n = lib().fav_flow_pairs_workspace_bytes_ex3(w, h, n_pairs, C.cast(C.pointer(o), C.c_void_p))
    if n == 0:
        _check(-1)
    return n


def flow_pairs(prev_list, cur_list, opts=None):
    """fav_flow_pairs_rgb8: both flows of every (prev[k], cur[k]) in one batched call -> (backward_list, forward_list), .flo payloads
    [H][W][2]: backward[k] is flow_rgb8(cur[k], prev[k]), forward[k] is flow_rgb8(prev[k], cur[k]), bit for bit.
    opts: a dict of levels, warps, iters, alpha, sweeps_per_launch, smooth_eps, data_term / gradient_data, match_beta, match_radius,
    median (0 / absent = default)."""
    torch = _torch()
    opts = dict(opts or {})
    n = len(prev_list)
    imgs = list(prev_list) + list(cur_list)
    if n != len(cur_list) or n == 0 or not all(t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 3 and
                                               t.shape == imgs[0].shape for t in imgs):
        raise FavError("flow_pairs: prev_list and cur_list must be equally long lists of contiguous uint8 CUDA tensors [H][W][3] of one size")
    h, w = imgs[0].shape[0], imgs[0].shape[1]
    o = _flow_opts_ex3(opts)
    nb = flow_pairs_workspace_bytes(w, h, n, **opts)
    ws = torch.empty(nb, dtype=torch.uint8, device=imgs[0].device)
    bw = [torch.empty((h, w, 2), dtype=torch.float32, device=imgs[0].device) for _ in range(n)]
    fw = [torch.empty((h, w, 2), dtype=torch.float32, device=imgs[0].device) for _ in range(n)]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    _check(lib().fav_flow_pairs_rgb8_ex3(arr(prev_list), arr(cur_list), n, w, h, C.byref(o), arr(bw), arr(fw), _p(ws), C.c_size_t(nb), _stream()))
    return bw, fw


def flow_median(flow, size: int):
    """fav_flow_median_f32: u and v of a flow [H][W][2], each replaced by the median of its size x size window (size 3 | 5, indices
    clamped to the image) -> a new tensor"""
    torch = _torch(); _chk_f32(flow, "flow")
    if flow.dim() != 3 or flow.shape[2] != 2:
        raise FavError("flow_median: flow must be [H][W][2]")
    h, w, _ = flow.shape
    out = torch.empty_like(flow)
    _check(lib().fav_flow_median_f32(_p(flow), _p(out), w, h, int(size), _stream()))
    return out


def flow_grey(rgb_hwc):
    torch = _torch()
    h, w = rgb_hwc.shape[0], rgb_hwc.shape[1]
    out = torch.empty((h, w), dtype=torch.float32, device=rgb_hwc.device)
    _check(lib().fav_flow_grey_f32(_p(rgb_hwc), _p(out), w, h, _stream()))
    return out


def flow_down(img):
    torch = _torch(); _chk_f32(img, "img")
    h, w = img.shape
    out = torch.empty(((h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=img.device)
    _check(lib().fav_flow_down_f32(_p(img), _p(out), w, h, _stream()))
    return out


def flow_up(coarse, h: int, w: int):
    torch = _torch(); _chk_f32(coarse, "coarse")
    out = torch.empty((h, w, 2), dtype=torch.float32, device=coarse.device)
    _check(lib().fav_flow_up_f32(_p(coarse), coarse.shape[1], coarse.shape[0], _p(out), w, h, _stream()))
    return out


def _flow_coef(kind: str, a_grey, b_grey, flow0, alpha: float, smooth_eps: float = 0.0):
    """fav_flow_coefficients<kind>_f32, kind "" | "_robust" | "_grad" -> (coef, weights): coef [5][H][W] for "_grad", else [H][W][4];
    weights [H][W][4] for "_robust" and with smooth_eps, else None.  (The plain entry takes neither smooth_eps nor weights.)"""
    torch = _torch(); _chk_f32(a_grey, "a_grey"); _chk_f32(b_grey, "b_grey"); _chk_f32(flow0, "flow0")
    h, w = a_grey.shape
    coef = torch.empty((5, h, w) if kind == "_grad" else (h, w, 4), dtype=torch.float32, device=a_grey.device)
    weights = torch.empty((h, w, 4), dtype=torch.float32, device=a_grey.device) if kind == "_robust" or smooth_eps else None
    args = [_p(a_grey), _p(b_grey), _p(flow0), C.c_float(alpha)] + ([C.c_float(smooth_eps), _p(coef), _p(weights)] if kind else [_p(coef)])
    _check(getattr(lib(), f"fav_flow_coefficients{kind}_f32")(*args, w, h, _stream()))
    return coef, weights


def _flow_sweeps(kind: str, flow0, coef, weights, iters: int, sweeps_per_launch: int):
    """fav_flow_sweeps<kind>_f32 (the plain entry takes no weights)"""
    torch = _torch(); _chk_f32(flow0, "flow0"); _chk_f32(coef, "coef")
    if weights is not None:
        _chk_f32(weights, "weights")
    h, w, _ = flow0.shape
    if kind == "_grad" and (tuple(coef.shape) != (5, h, w) or (weights is not None and tuple(weights.shape) != (h, w, 4))):
        raise FavError("flow_sweeps_grad: coef must be [5][H][W] and weights [H][W][4] for a flow [H][W][2]")
    out, scratch = torch.empty_like(flow0), torch.empty_like(flow0)
    args = [_p(flow0), _p(coef)] + ([_p(weights)] if kind else [])
    _check(getattr(lib(), f"fav_flow_sweeps{kind}_f32")(*args, iters, sweeps_per_launch, _p(out), _p(scratch), w, h, _stream()))
    return out


def flow_coefficients(a_grey, b_grey, flow0, alpha: float = 15.0):
    return _flow_coef("", a_grey, b_grey, flow0, alpha)[0]


def flow_sweeps(flow0, coef, iters: int, sweeps_per_launch: int = 0):
    return _flow_sweeps("", flow0, coef, None, iters, sweeps_per_launch)


def flow_coefficients_robust(a_grey, b_grey, flow0, alpha: float = 5.0, smooth_eps: float = 0.3):
    """one warp of the edge-preserving smoothness -> (coef [H][W][4] = (a, b, c, r), weights [H][W][4] = (n_l, n_r, n_u, n_d))"""
    return _flow_coef("_robust", a_grey, b_grey, flow0, alpha, smooth_eps)


def flow_sweeps_robust(flow0, coef, weights, iters: int, sweeps_per_launch: int = 0):
    _chk_f32(weights, "weights")
    return _flow_sweeps("_robust", flow0, coef, weights, iters, sweeps_per_launch)


def flow_coefficients_grad(a_grey, b_grey, flow0, alpha: float = 8.0, smooth_eps: float = 0.0):
    """one warp of the gradient-constancy data term -> coef [5][H][W] = the planes (q11, q12, q22, e1, e2); with smooth_eps > 0 (the
    edge-preserving smoothness) -> (coef, weights [H][W][4] = (n_l, n_r, n_u, n_d))"""
    coef, weights = _flow_coef("_grad", a_grey, b_grey, flow0, alpha, smooth_eps)
    return (coef, weights) if smooth_eps else coef


def flow_match(a_grey, b_grey, radius: int = 16):
    """fav_flow_match_f32: the block-matching fields of two grey planes [H][W], both directions -> (d_ab, d_ba), int16 [H][W][2] (dx, dy)"""
    torch = _torch(); _chk_f32(a_grey, "a_grey"); _chk_f32(b_grey, "b_grey")
    if a_grey.dim() != 2 or a_grey.shape != b_grey.shape:
        raise FavError("flow_match: a_grey and b_grey must be [H][W] of one size")
    h, w = a_grey.shape
    d_ab = torch.empty((h, w, 2), dtype=torch.int16, device=a_grey.device); d_ba = torch.empty_like(d_ab)
    _check(lib().fav_flow_match_f32(_p(a_grey), _p(b_grey), w, h, int(radius), _p(d_ab), _p(d_ba), _stream()))
    return d_ab, d_ba


def flow_match_check(d_ab, d_ba, want_prior: bool = False):
    """fav_flow_match_check: the forward-backward test of two match fields -> m [H][W] (0 | 1, fp32); want_prior: the three planes
    [3][H][W] = (d_ab.x, d_ab.y, m) that fav_flow_coefficients_prior_f32 takes"""
    torch = _torch()
    if not (d_ab.is_cuda and d_ba.is_cuda and d_ab.dtype == torch.int16 and d_ba.dtype == torch.int16 and d_ab.is_contiguous() and d_ba.is_contiguous() and
            d_ab.dim() == 3 and d_ab.shape[2] == 2 and d_ab.shape == d_ba.shape):
        raise FavError("flow_match_check: d_ab and d_ba must be contiguous int16 CUDA tensors [H][W][2] of one size")
    h, w, _ = d_ab.shape
    prior = torch.empty((3, h, w), dtype=torch.float32, device=d_ab.device)
    _check(lib().fav_flow_match_check(_p(d_ab), _p(d_ba), w, h, _p(prior), _stream()))
    return prior if want_prior else prior[2]


def scene_change_workspace_bytes() -> int:
    return lib().fav_scene_change_workspace_bytes()


def scene_change(prev, cur, workspace=None, result=None, workspace_bytes: Optional[int] = None, w: Optional[int] = None, h: Optional[int] = None):
    """fav_scene_change_rgb8: the block-histogram distance of two u8 [H][W][3] frames -> (total, cells), `cells` the 16 per-cell sums
    (index cy*4+cx) as a list; the score is total / (2 W H).  workspace: a CUDA tensor of at least scene_change_workspace_bytes() bytes to
    use (workspace_bytes: the size to declare instead of its own); result: an int32 tensor of 17 elements to write into -- CUDA, or
    pinned host memory, which the device writes through its mapping; w, h: the size to declare instead of the tensors' own."""
    torch = _torch()
    for t in (prev, cur):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 3 and t.shape == prev.shape):
            raise FavError("scene_change: prev and cur must be contiguous uint8 CUDA tensors [H][W][3] of one size")
    if workspace is None:
        workspace = torch.empty((scene_change_workspace_bytes(),), dtype=torch.uint8, device=prev.device)
    if result is None:
        result = torch.empty((17,), dtype=torch.int32, device=prev.device)
    if not (result.dtype == torch.int32 and result.numel() >= 17 and result.is_contiguous() and (result.is_cuda or result.is_pinned())):
        raise FavError("scene_change: result must be a contiguous int32 tensor of 17 elements, CUDA or pinned")
    nbytes = workspace.numel() * workspace.element_size() if workspace_bytes is None else workspace_bytes
    _check(lib().fav_scene_change_rgb8(_p(prev), _p(cur), prev.shape[1] if w is None else w, prev.shape[0] if h is None else h,
                                       _p(workspace), C.c_size_t(nbytes), _p(result), _stream()))
    if not result.is_cuda:
        torch.cuda.current_stream().synchronize()
    r = result.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return int(r[0]), [int(v) for v in r[1:17]]


def flow_coefficients_prior(a_grey, b_grey, flow0, prior, alpha: float, beta: float = 225.0, tau: float = 1.0, smooth_eps: float = 0.0, data_term: int = 0):
    """fav_flow_coefficients_prior_f32: one warp's coefficients with the matching prior `prior` [3][Hp][Wp] (the level's own size, or
    the next coarser level's: level 0 reading level 1) -> coef [5][H][W] (smooth_eps == 0) or (coef, weights [H][W][4])"""
    torch = _torch(); _chk_f32(a_grey, "a_grey"); _chk_f32(b_grey, "b_grey"); _chk_f32(flow0, "flow0"); _chk_f32(prior, "prior")
    h, w = a_grey.shape
    if prior.dim() != 3 or prior.shape[0] != 3 or tuple(flow0.shape) != (h, w, 2) or b_grey.shape != a_grey.shape:
        raise FavError("flow_coefficients_prior: prior must be [3][Hp][Wp], flow0 [H][W][2], the grey planes [H][W]")
    coef = torch.empty((5, h, w), dtype=torch.float32, device=a_grey.device)
    weights = torch.empty((h, w, 4), dtype=torch.float32, device=a_grey.device) if smooth_eps > 0 else None
    _check(lib().fav_flow_coefficients_prior_f32(_p(a_grey), _p(b_grey), _p(flow0), C.c_float(alpha), C.c_float(smooth_eps), int(data_term), _p(prior),
                                                 prior.shape[2], prior.shape[1], C.c_float(beta), C.c_float(tau), _p(coef), _p(weights), w, h, _stream()))
    return (coef, weights) if smooth_eps > 0 else coef


def flow_sweeps_grad(flow0, coef, iters: int, sweeps_per_launch: int = 0, weights=None):
    """`iters` sweeps of the tensor form; coef [5][H][W]; weights: the [H][W][4] of the weighted mean, None for the plain mean"""
    return _flow_sweeps("_grad", flow0, coef, weights, iters, sweeps_per_launch)


# ------------------------------------------------------------------------------------------------ network
class Net:
    def __init__(self, t7_path: Optional[str] = None, device: int = 0, blob: Optional[bytes] = None):
        h = C.c_void_p()
        if blob is not None:
            _check(lib().fav_net_create_from_blob(blob, C.c_size_t(len(blob)), device, C.byref(h)))
        else:
            _check(lib().fav_net_create(t7_path.encode(), device, C.byref(h)))
        self.h, self.device = h, device
        self._users, self._close_pending = 0, False

    # A fav_stream / fav_vr reads its network when it is destroyed (~fav_stream, ~fav_vr select the network's device), so the network must
    # outlive the objects built on it.  Reference counting sees to that as long as finalisers run in order, but the garbage collector
    # finalises the members of a reference cycle in ANY order (a test's frame kept alive by a caught exception is such a cycle): a Net
    # that is closed while Streams / VRs still use it is therefore destroyed when the last of them has been.
    def _retain(self):
        self._users += 1

    def _release(self):
        self._users -= 1
        if self._users == 0 and self._close_pending:
            self.close()

    def close(self):
        if getattr(self, "_users", 0) > 0:
            self._close_pending = True
            return
        if getattr(self, "h", None) and lib is not None:
            try:
                lib().fav_net_destroy(self.h)
            except Exception:      # interpreter shutdown
                pass
            self.h = None

    __del__ = close

    def check(self):
        """fav_net_check: raises if a stream-K hand-off timed out since the last check (call after synchronising)"""
        _torch().cuda.synchronize()
        _check(lib().fav_net_check(self.h))

    def set_shared_device(self, shared: bool):
        """True: data-parallel convolution grids only (no stream-K hand-offs): for a GPU this process does not own exclusively"""
        _check(lib().fav_net_set_shared_device(self.h, 1 if shared else 0))

    def set_precision(self, bf16_operands: bool):
        """False: fp32 parity mode (default); True: bf16 operands in the 3x3 halo convolutions (fast mode, not bit-compatible)."""
        _check(lib().fav_net_set_precision(self.h, 1 if bf16_operands else 0))

    def describe(self) -> str:
        buf = C.create_string_buffer(1 << 16)
        _check(lib().fav_net_describe_host(self.h, buf, C.c_size_t(len(buf))))
        return buf.value.decode()

    def input_pad(self) -> int:
        """the leading reflection padding the input assembly writes itself (fav_net::upload: a first layer `pad p p p p`), else 0"""
        first = self.describe().split("\n", 1)[0].split()
        return int(first[1]) if first[:1] == ["pad"] and len(set(first[1:])) == 1 else 0

    def param_count(self) -> int:
        return int(lib().fav_net_param_count(self.h))

    def output_size(self, h: int, w: int) -> Tuple[int, int]:
        ho, wo = C.c_int(), C.c_int()
        _check(lib().fav_net_output_size(self.h, h, w, C.byref(ho), C.byref(wo)))
        return ho.value, wo.value

    def profile_enable(self, on: bool = True):
        _check(lib().fav_net_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        """[(ms_sum, launches, useful_macs_per_launch, n_tile)] per convolution, network order"""
        cap = 256
        cnt = C.c_int(); ms = (C.c_double * cap)(); n = (C.c_int * cap)(); macs = (C.c_double * cap)(); tile = (C.c_int * cap)()
        _check(lib().fav_net_profile_read_host(self.h, cap, C.byref(cnt), ms, n, macs, tile))
        return [(ms[i], n[i], macs[i], tile[i]) for i in range(cnt.value)]

    def forward(self, in7):
        torch = _torch(); _chk_f32(in7, "in7")
        x = in7[0] if in7.dim() == 4 else in7
        _, h, w = x.shape
        ho, wo = self.output_size(h, w)
        out = torch.empty((3, ho, wo), dtype=torch.float32, device=x.device)
        _check(lib().fav_net_forward(self.h, _p(x), _p(out), h, w, _stream()))
        return out[None] if in7.dim() == 4 else out


def describe_t7(t7_path: str) -> str:
    """host-only: layer list as parsed by the product's C++ .t7 reader"""
    buf = C.create_string_buffer(1 << 16)
    _check(lib().fav_t7_describe_host(t7_path.encode(), buf, C.c_size_t(len(buf))))
    return buf.value.decode()


def describe_layers(layers, indent: int = 0) -> str:
    """the same text from the Python reader's layer list (fav_amd.t7.extract_layers)"""
    out = []
    pad = "  " * indent
    for L in layers:
        t = L["type"]
        if t == "pad": out.append(f"{pad}{'replicate-pad' if L.get('mode') == 'replicate' else 'pad'} {L['l']} {L['r']} {L['t']} {L['b']}")
        elif t == "fullconv":
            ci, co, k, _ = L["w"].shape
            out.append(f"{pad}fullconv {ci} {co} {k} {L['stride']} {L['pad']} adj={L['adj']} bias={0 if L['b'] is None else 1}")
        elif t == "bn": out.append(f"{pad}bn {len(L['mean'])}")
        elif t == "conv":
            co, ci, k, _ = L["w"].shape
            out.append(f"{pad}conv {ci} {co} {k} {L['stride']} {L['pad']} bias={0 if L['b'] is None else 1}")
        elif t == "in": out.append(f"{pad}in {len(L['gamma'])}")
        elif t == "relu": out.append(f"{pad}relu")
        elif t == "res":
            out.append(f"{pad}res shave={L['shave']}"); out.append(describe_layers(L["block"], indent + 1).rstrip("\n"))
        elif t == "up": out.append(f"{pad}up {L['s']}")
        elif t == "tanh": out.append(f"{pad}tanh")
        elif t == "mul": out.append(f"{pad}mul {L['k']:g}")
        else: out.append(f"{pad}identity")
    return "\n".join(out) + "\n"


def pack_checkpoint(t7_path: str) -> bytes:
    n = C.c_size_t()
    _check(lib().fav_net_pack_host(t7_path.encode(), None, C.c_size_t(0), C.byref(n)))
    buf = C.create_string_buffer(n.value)
    _check(lib().fav_net_pack_host(t7_path.encode(), buf, C.c_size_t(n.value), C.byref(n)))
    return buf.raw[:n.value]


class _Opts(C.Structure):
    _fields_ = [("border_mode", C.c_int), ("occlusions_min_filter", C.c_int), ("invert_occlusion", C.c_int),
                ("fix_occlusions", C.c_int), ("fill_random", C.c_int), ("seed", C.c_uint)]


class Stream:
    """One video stream: the recurrent per-frame pipeline (fast_artistic_video_core.lua:194-211)."""

    def __init__(self, net: Net, h: int, w: int, border: int = BORDER_STN, min_filter_r: int = 7,
                 invert_occlusion: bool = False, fix_occlusions: bool = False, fill_random: bool = False, seed: int = 1):
        self.net, self.H, self.W = net, h, w
        self._img = None
        o = _Opts(border, min_filter_r, int(invert_occlusion), int(fix_occlusions), int(fill_random), seed)
        hd = C.c_void_p()
        _check(lib().fav_stream_create(net.h, h, w, C.byref(o), C.byref(hd)))
        self.h = hd
        net._retain()
        ho, wo = C.c_int(), C.c_int()
        _check(lib().fav_stream_output_size(hd, C.byref(ho), C.byref(wo)))
        self.Ho, self.Wo = ho.value, wo.value          # size of the stylised frames (= H x W when both are multiples of 4)

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            try:
                lib().fav_stream_destroy(self.h)
            except Exception:      # interpreter shutdown
                pass
            self.h = None
            self.net._release()
            if self._img is not None:
                self._img._release()

    __del__ = close

    def set_image_net(self, img_net: Optional[Net]):
        _check(lib().fav_stream_set_image_net(self.h, img_net.h if img_net is not None else None))
        if img_net is not None:
            img_net._retain()
        if self._img is not None:
            self._img._release()
        self._img = img_net      # keep alive

    def set_single_image_size(self, hs: int, ws: int):
        """-scale_factor: frames without a prior run at hs x ws and are scaled back to H x W (0, 0: the unscaled path)"""
        _check(lib().fav_stream_set_single_image_size(self.h, hs, ws))

    def _outs(self, dev, want_f32, want_u8):
        torch = _torch()
        f = torch.empty((3, self.Ho, self.Wo), dtype=torch.float32, device=dev) if want_f32 else None
        u = torch.empty((self.Ho, self.Wo, 3), dtype=torch.uint8, device=dev) if want_u8 else None
        return f, u

    def first_frame(self, frame_u8_hwc, want_f32=True, want_u8=False, out_f32=None, out_u8=None):
        f, u = self._outs(frame_u8_hwc.device, want_f32 and out_f32 is None, want_u8 and out_u8 is None)
        f = out_f32 if out_f32 is not None else f; u = out_u8 if out_u8 is not None else u
        _check(lib().fav_stream_first_frame(self.h, _p(frame_u8_hwc), _p(f), _p(u), _stream()))
        return f, u

    def next_frame_cert(self, frame_u8_hwc, backward_flo, cert_u8, want_f32=True, want_u8=False, out_f32=None, out_u8=None):
        f, u = self._outs(frame_u8_hwc.device, want_f32 and out_f32 is None, want_u8 and out_u8 is None)
        f = out_f32 if out_f32 is not None else f; u = out_u8 if out_u8 is not None else u
        _check(lib().fav_stream_next_frame_cert(self.h, _p(frame_u8_hwc), _p(backward_flo), _p(cert_u8), _p(f), _p(u), _stream()))
        return f, u

    def next_frame_flow(self, frame_u8_hwc, backward_flo, forward_flo, use_structure=False, want_f32=True, want_u8=False,
                        out_f32=None, out_u8=None):
        f, u = self._outs(frame_u8_hwc.device, want_f32 and out_f32 is None, want_u8 and out_u8 is None)
        f = out_f32 if out_f32 is not None else f; u = out_u8 if out_u8 is not None else u
        _check(lib().fav_stream_next_frame_flow(self.h, _p(frame_u8_hwc), _p(backward_flo), _p(forward_flo),
                                                1 if use_structure else 0, _p(f), _p(u), _stream()))
        return f, u

    def next_frame_estimate(self, frame_u8_hwc, prev_frame_u8_hwc, use_structure=False, want_f32=True, want_u8=False, batched=False, **flow_opts):
        """fav_stream_next_frame_estimate (the -estimate_flow path): both flows from the two frames, then next_frame_flow.
        batched: pass the workspace of the batch of one (flow_pairs_workspace_bytes), as bin/fav_stylize does -- the same bits.
        Returns (f32, u8, backward_flo, forward_flo)."""
        torch = _torch()
        f, u = self._outs(frame_u8_hwc.device, want_f32, want_u8)
        o = _flow_opts_ex3(flow_opts)
        nb = flow_pairs_workspace_bytes(self.W, self.H, 1, **flow_opts) if batched else flow_workspace_bytes(self.W, self.H, **flow_opts)
        ws = torch.empty(nb, dtype=torch.uint8, device=frame_u8_hwc.device)
        bw = torch.empty((self.H, self.W, 2), dtype=torch.float32, device=frame_u8_hwc.device)
        fw = torch.empty_like(bw)
        _check(lib().fav_stream_next_frame_estimate_ex3(self.h, _p(frame_u8_hwc), _p(prev_frame_u8_hwc), C.byref(o), 1 if use_structure else 0,
                                                       _p(bw), _p(fw), _p(ws), C.c_size_t(nb), _p(f), _p(u), _stream()))
        return f, u, bw, fw

    def set_long_term(self, distances):
        """fav_stream_set_long_term: long-term priors from the stylised frames at these distances (ascending, the first one 1; () = off)"""
        d = [int(x) for x in distances]
        _check(lib().fav_stream_set_long_term(self.h, (C.c_int * max(len(d), 1))(*d), len(d)))

    def long_term_available(self) -> int:
        return lib().fav_stream_long_term_available(self.h)

    def next_frame_flows_lt(self, frame_u8_hwc, backward_flos, forward_flos, use_structure=False, want_f32=True, want_u8=False):
        """fav_stream_next_frame_flows_lt: the next frame from the flows of the first len(backward_flos) configured distances"""
        f, u = self._outs(frame_u8_hwc.device, want_f32, want_u8)
        _check(lib().fav_stream_next_frame_flows_lt(self.h, _p(frame_u8_hwc), len(backward_flos), _ptr_array(backward_flos), _ptr_array(forward_flos),
                                                    1 if use_structure else 0, _p(f), _p(u), _stream()))
        return f, u

    def long_term_workspace_bytes(self, **flow_opts) -> int:
        o = _flow_opts_ex3(flow_opts)
        n = lib().fav_stream_long_term_workspace_bytes(self.h, C.cast(C.pointer(o), C.c_void_p))
        if n == 0:
            _check(-1)
        return n

    def next_frame_estimate_lt(self, frame_u8_hwc, use_structure=False, want_f32=True, want_u8=False, workspace=None, **flow_opts):
        """fav_stream_next_frame_estimate_lt: the next frame from the frames alone, flows to every distance the history serves.
        Returns (f32, u8, backward_flos, forward_flos): the flows are views into the workspace, one pair per distance used."""
        torch = _torch()
        f, u = self._outs(frame_u8_hwc.device, want_f32, want_u8)
        o = _flow_opts_ex3(flow_opts)
        nb = self.long_term_workspace_bytes(**flow_opts)
        ws = workspace if workspace is not None else torch.empty(nb, dtype=torch.uint8, device=frame_u8_hwc.device)
        m = self.long_term_available()      # (right after set_state fewer distances hold a frame: their views are not written)
        _check(lib().fav_stream_next_frame_estimate_lt(self.h, _p(frame_u8_hwc), C.byref(o), 1 if use_structure else 0, _p(ws), C.c_size_t(ws.numel()),
                                                       _p(f), _p(u), _stream()))
        fb = (self.H * self.W * 8 + 255) // 256 * 256
        view = lambda j: ws[j * fb:j * fb + self.H * self.W * 8].view(torch.float32).view(self.H, self.W, 2)
        return f, u, [view(2 * k) for k in range(m)], [view(2 * k + 1) for k in range(m)]

    def prefetch_mask(self, frame_u8_hwc, backward_flo, forward_flo, use_structure=False):
        _check(lib().fav_stream_prefetch_mask(self.h, _p(frame_u8_hwc), _p(backward_flo), _p(forward_flo),
                                              1 if use_structure else 0, _stream()))

    def state(self):
        torch = _torch()
        out = torch.empty((3, self.Ho, self.Wo), dtype=torch.float32, device=f"cuda:{self.net.device}")
        _check(lib().fav_stream_get_state(self.h, _p(out), _stream()))
        return out

    def set_state(self, t):
        _chk_f32(t, "state")
        _check(lib().fav_stream_set_state(self.h, _p(t), _stream()))

    def set_host_ordered(self, on: bool):
        """look-ahead without events: the caller synchronises the inputs itself before prefetch_mask (see include/fav.h)"""
        _check(lib().fav_stream_set_host_ordered(self.h, 1 if on else 0))

    def png_buffers(self):
        """(out, nbytes) device buffers for encode_png_into: capacity fav_png_capacity(W, H), one int32"""
        torch = _torch()
        cap = lib().fav_png_capacity(self.Wo, self.Ho)
        dev = torch.device("cuda", self.net.device)
        return torch.empty((cap + 3) // 4 * 4, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def encode_png_into(self, out, nbytes):
        """fav_stream_encode_png: the current stylised frame as the bytes of a PNG file, enqueued on the current stream (no sync)"""
        _check(lib().fav_stream_encode_png(self.h, _p(out), C.c_size_t(out.numel()), _p(nbytes), _stream()))

    def encode_png_async_into(self, out, nbytes):
        """fav_stream_encode_png_async: the same bytes, produced on the stream's own encoder queue next to the following frame"""
        _check(lib().fav_stream_encode_png_async(self.h, _p(out), C.c_size_t(out.numel()), _p(nbytes), _stream()))

    def wait_png(self):
        """fav_stream_wait_png: the current stream waits for the asynchronous encodes issued so far"""
        _check(lib().fav_stream_wait_png(self.h, _stream()))

    def encode_yuv_into(self, out, fmt: "YuvFormat", capacity: Optional[int] = None):
        """fav_stream_encode_yuv: the current stylised frame as the planes of a Y4M frame, enqueued on the current stream (no sync)"""
        _check(lib().fav_stream_encode_yuv(self.h, C.byref(fmt), _p(out), C.c_size_t(out.numel() if capacity is None else capacity), _stream()))

    def encode_png_colors_into(self, frame_u8_hwc, matrix: int, out, nbytes):
        """fav_stream_encode_png_colors: the current stylised frame's luminance on the colours of frame_u8_hwc, as the bytes of a PNG file"""
        _check(lib().fav_stream_encode_png_colors(self.h, _p(frame_u8_hwc), matrix, _p(out), C.c_size_t(out.numel()), _p(nbytes), _stream()))

    def encode_yuv_layout_into(self, out, layout: "YuvLayout", capacity: Optional[int] = None):
        """fav_stream_encode_yuv_layout: the current stylised frame as planes of any layout (above 8 bits: unquantised floats in),
        enqueued on the current stream (no sync).  out: a u8 tensor; capacity in bytes"""
        _check(lib().fav_stream_encode_yuv_layout(self.h, C.byref(layout), _p(out), C.c_size_t(out.numel() if capacity is None else capacity), _stream()))

    def encode_yuv_colors_into(self, frame_u8_hwc, out, fmt: "YuvFormat", capacity: Optional[int] = None):
        """fav_stream_encode_yuv_colors: the planes of that image (the transfer takes fmt's matrix), enqueued on the current stream (no sync)"""
        _check(lib().fav_stream_encode_yuv_colors(self.h, _p(frame_u8_hwc), C.byref(fmt), _p(out),
                                                  C.c_size_t(out.numel() if capacity is None else capacity), _stream()))

    def last_input(self):
        """[7][H][W] network input of the last frame (content | prior | certainty), un-padded copy of the fused kernel's output"""
        torch = _torch()
        out = torch.empty((7, self.H, self.W), dtype=torch.float32, device=f"cuda:{self.net.device}")
        _check(lib().fav_stream_get_input_f32(self.h, _p(out), _stream()))
        return out

    def last_padded_input(self):
        """[H + 2p][W + 2p][8] network input of the last frame as the network reads it: the stream's own buffer with the leading reflection
        padding p (Net.input_pad) and the zero eighth channel, copied device to device"""
        torch = _torch()
        p = self.net.input_pad()
        out = torch.empty((self.H + 2 * p, self.W + 2 * p, 8), dtype=torch.float32, device=f"cuda:{self.net.device}")
        _check(lib().fav_stream_get_padded_input_f32(self.h, _p(out), _stream()))
        return out

    def last_mask(self):
        """copy of the u8 certainty mask used for the last frame (before the min filter)"""
        torch = _torch()
        ptr = lib().fav_stream_last_mask(self.h)
        out = torch.empty((self.H, self.W), dtype=torch.uint8, device=f"cuda:{self.net.device}")
        # device-to-device copy through torch's runtime (same HIP context)
        src = _from_ptr_u8(ptr, self.H * self.W, self.net.device)
        out.view(-1).copy_(src)
        return out


def png_encode(img, from_stream: "Stream" = None) -> bytes:
    """A9 on the GPU: the bytes of the PNG file (fav_png_encode_rgb8 for a u8 [H][W][3] tensor, fav_png_encode_f32 for a float
    [3][H][W] tensor, fav_stream_encode_png for a Stream's current frame)."""
    torch = _torch()
    if from_stream is not None:
        h, w, dev = from_stream.Ho, from_stream.Wo, torch.device("cuda", from_stream.net.device)
    elif img.dtype == torch.uint8:
        h, w, dev = img.shape[0], img.shape[1], img.device
    else:
        h, w, dev = img.shape[1], img.shape[2], img.device
    cap = lib().fav_png_capacity(w, h)
    out = torch.empty((cap + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    nbytes = torch.zeros(1, dtype=torch.int32, device=dev)
    if from_stream is not None:
        _check(lib().fav_stream_encode_png(from_stream.h, _p(out), C.c_size_t(cap), _p(nbytes), _stream()))
    else:
        wsb = lib().fav_png_workspace_bytes(w, h)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        assert img.is_contiguous()
        fn = lib().fav_png_encode_rgb8 if img.dtype == torch.uint8 else lib().fav_png_encode_f32
        _check(fn(_p(img), w, h, _p(out), C.c_size_t(cap), _p(nbytes), _p(ws), C.c_size_t(wsb), _stream()))
    torch.cuda.synchronize()
    n = int(nbytes.item())
    return bytes(out[:n].cpu().numpy().tobytes())


# ---- YUV4MPEG2: 8-bit YCbCr planes <-> RGB (fav_yuv_*, fav_y4m_*)
YUV_420, YUV_444 = 0, 1
YUV_SITING_CENTER, YUV_SITING_LEFT = 0, 1
YUV_BT601, YUV_BT709 = 0, 1


class YuvFormat(C.Structure):
    """fav_yuv_format"""
    _fields_ = [("chroma", C.c_int), ("siting", C.c_int), ("matrix", C.c_int), ("full_range", C.c_int)]

    def __repr__(self):
        return f"YuvFormat(chroma={self.chroma}, siting={self.siting}, matrix={self.matrix}, full_range={self.full_range})"


class Y4mHeader(C.Structure):
    """fav_y4m_header"""
    _fields_ = [("W", C.c_int), ("H", C.c_int), ("fps_num", C.c_int), ("fps_den", C.c_int), ("aspect_num", C.c_int),
                ("aspect_den", C.c_int), ("interlace", C.c_int), ("fmt", YuvFormat), ("xtags", C.c_char * 1024)]


def yuv_format(chroma: int = YUV_420, siting: int = YUV_SITING_CENTER, matrix: int = YUV_BT601, full_range: bool = False) -> YuvFormat:
    return YuvFormat(chroma, siting, matrix, int(full_range))


def yuv_frame_bytes(w: int, h: int, fmt: YuvFormat) -> int:
    """bytes of one frame's payload; raises on a bad size or format"""
    n = lib().fav_yuv_frame_bytes(w, h, C.byref(fmt))
    if n == 0:
        raise FavError(lib().fav_last_error().decode(errors="replace"))
    return n


def yuv_to_rgb8(yuv, w: int, h: int, fmt: YuvFormat, out=None):
    """fav_yuv_to_rgb8: a frame's planes (flat u8 tensor) -> [H][W][3] u8.  out: a u8 tensor of at least H*W*3 elements to write into"""
    torch = _torch()
    assert yuv.dtype == torch.uint8 and yuv.is_contiguous() and yuv.numel() >= yuv_frame_bytes(w, h, fmt)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=yuv.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= h * w * 3
    _check(lib().fav_yuv_to_rgb8(_p(yuv), w, h, C.byref(fmt), _p(out), _stream()))
    return out


def rgb_to_yuv(img, fmt: YuvFormat, out=None):
    """fav_rgb8_to_yuv for a u8 [H][W][3] tensor, fav_rgb_f32_to_yuv for a float [3][H][W] tensor (image.save's quantisation in front)
    -> the frame's planes, flat u8.  out: a u8 tensor of at least fav_yuv_frame_bytes elements to write into"""
    torch = _torch()
    assert img.is_contiguous()
    u8 = img.dtype == torch.uint8
    h, w = (img.shape[0], img.shape[1]) if u8 else (img.shape[1], img.shape[2])
    n = yuv_frame_bytes(w, h, fmt)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=img.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= n
    if not u8:
        _chk_f32(img, "img")
    _check((lib().fav_rgb8_to_yuv if u8 else lib().fav_rgb_f32_to_yuv)(_p(img), w, h, C.byref(fmt), _p(out), _stream()))
    return out


def color_transfer(stylised, original, matrix_or_fmt, out=None):
    """-original_colors: the luminance of `stylised` (float [3][H][W], image.save's quantisation in front) on the colours of `original`
    (u8 [H][W][3]).  An int matrix (YUV_BT601 | YUV_BT709): fav_color_transfer_rgb8 -> [H][W][3] u8; a YuvFormat: fav_color_transfer_yuv
    -> the planes of that image, flat u8.  out: a u8 tensor of at least H*W*3 / fav_yuv_frame_bytes elements to write into"""
    torch = _torch()
    _chk_f32(stylised, "stylised")
    h, w = stylised.shape[1], stylised.shape[2]
    assert original.dtype == torch.uint8 and original.is_contiguous() and original.numel() >= h * w * 3
    planes = isinstance(matrix_or_fmt, YuvFormat)
    n = yuv_frame_bytes(w, h, matrix_or_fmt) if planes else h * w * 3
    if out is None:
        out = torch.empty(n if planes else (h, w, 3), dtype=torch.uint8, device=stylised.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= n
    if planes:
        _check(lib().fav_color_transfer_yuv(_p(stylised), _p(original), w, h, C.byref(matrix_or_fmt), _p(out), _stream()))
    else:
        _check(lib().fav_color_transfer_rgb8(_p(stylised), _p(original), w, h, int(matrix_or_fmt), _p(out), _stream()))
    return out


def y4m_parse_header(line: bytes) -> Y4mHeader:
    """fav_y4m_parse_header_host (no device needed); raises FavError with the library's message"""
    h = Y4mHeader()
    _check(lib().fav_y4m_parse_header_host(line, C.c_size_t(len(line)), C.byref(h)))
    return h


def y4m_format_header(h: Y4mHeader) -> bytes:
    """fav_y4m_format_header_host (no device needed): the header line, newline included"""
    buf = C.create_string_buffer(1100)
    n = lib().fav_y4m_format_header_host(C.byref(h), buf, C.c_size_t(len(buf)))
    if n <= 0:
        _check(n if n else -1)
    return buf.raw[:n]


# ---- include/fav_yuv.h: every layout (4:2:0, 4:2:2, 4:4:4 at 8, 9, 10, 12, 14, 16 bits); planes travel as flat u8 tensors of
# fav_yuv_layout_frame_bytes BYTES (a sample above 8 bits is two of them, little-endian) at any byte offset
YUV_422 = 2


class YuvLayout(C.Structure):
    """fav_yuv_layout"""
    _fields_ = [("struct_bytes", C.c_uint32), ("chroma", C.c_int), ("siting", C.c_int), ("matrix", C.c_int), ("full_range", C.c_int),
                ("depth", C.c_int)]

    def __repr__(self):
        return (f"YuvLayout(chroma={self.chroma}, siting={self.siting}, matrix={self.matrix}, full_range={self.full_range}, "
                f"depth={self.depth})")


class Y4mStreamHeader(C.Structure):
    """fav_y4m_stream_header"""
    _fields_ = [("W", C.c_int), ("H", C.c_int), ("fps_num", C.c_int), ("fps_den", C.c_int), ("aspect_num", C.c_int),
                ("aspect_den", C.c_int), ("interlace", C.c_int), ("layout", YuvLayout), ("xtags", C.c_char * 1024)]


def yuv_layout(chroma: int = YUV_420, siting: int = YUV_SITING_CENTER, matrix: int = YUV_BT601, full_range: bool = False, depth: int = 8,
               struct_bytes: Optional[int] = None) -> YuvLayout:
    return YuvLayout(C.sizeof(YuvLayout) if struct_bytes is None else struct_bytes, chroma, siting, matrix, int(full_range), depth)


def yuv_layout_frame_bytes(w: int, h: int, layout: YuvLayout) -> int:
    """bytes of one frame's payload; raises on a bad size or field"""
    n = lib().fav_yuv_layout_frame_bytes(w, h, C.byref(layout))
    if n == 0:
        raise FavError(lib().fav_last_error().decode(errors="replace"))
    return n


def yuv_layout_to_rgb8(yuv, w: int, h: int, layout: YuvLayout, out=None):
    """fav_yuv_layout_to_rgb8: a frame's planes (flat u8 tensor of its bytes) -> [H][W][3] u8.  out: a u8 tensor of at least H*W*3 elements"""
    torch = _torch()
    assert yuv.dtype == torch.uint8 and yuv.is_contiguous() and yuv.numel() >= yuv_layout_frame_bytes(w, h, layout)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=yuv.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= h * w * 3
    _check(lib().fav_yuv_layout_to_rgb8(_p(yuv), w, h, C.byref(layout), _p(out), _stream()))
    return out


def rgb_to_yuv_layout(img, layout: YuvLayout, out=None):
    """fav_rgb8_to_yuv_layout for a u8 [H][W][3] tensor, fav_rgb_f32_to_yuv_layout for a float [3][H][W] tensor (depth 8: image.save's
    quantisation in front; deeper: unquantised) -> the frame's planes, flat u8 of fav_yuv_layout_frame_bytes bytes"""
    torch = _torch()
    assert img.is_contiguous()
    u8 = img.dtype == torch.uint8
    h, w = (img.shape[0], img.shape[1]) if u8 else (img.shape[1], img.shape[2])
    n = yuv_layout_frame_bytes(w, h, layout)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=img.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= n
    if not u8:
        _chk_f32(img, "img")
    _check((lib().fav_rgb8_to_yuv_layout if u8 else lib().fav_rgb_f32_to_yuv_layout)(_p(img), w, h, C.byref(layout), _p(out), _stream()))
    return out


def y4m_parse_stream_header(line: bytes) -> Y4mStreamHeader:
    """fav_y4m_parse_stream_header_host (no device needed); raises FavError with the library's message"""
    h = Y4mStreamHeader()
    _check(lib().fav_y4m_parse_stream_header_host(line, C.c_size_t(len(line)), C.byref(h)))
    return h


def y4m_format_stream_header(h: Y4mStreamHeader) -> bytes:
    """fav_y4m_format_stream_header_host (no device needed): the header line, newline included"""
    buf = C.create_string_buffer(1100)
    n = lib().fav_y4m_format_stream_header_host(C.byref(h), buf, C.c_size_t(len(buf)))
    if n <= 0:
        _check(n if n else -1)
    return buf.raw[:n]


def png_tables():
    """the encoder's Huffman codes (host-only): list of dicts {len[277], code[277], hdr (uint32 words), hdr_bits, btype, dist_len, dist_code}"""
    cnt, tb = C.c_int(), C.c_int()
    _check(lib().fav_png_tables_host(None, C.c_size_t(0), C.byref(cnt), C.byref(tb)))
    buf = np.zeros(cnt.value * tb.value // 4, np.uint32)
    _check(lib().fav_png_tables_host(buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes), C.byref(cnt), C.byref(tb)))
    out = []
    w = tb.value // 4
    for k in range(cnt.value):
        t = buf[k * w:(k + 1) * w]
        out.append({"len": (t[:277] >> 16).astype(int), "code": (t[:277] & 0xFFFF).astype(int), "hdr": t[277:277 + 40].copy(),
                    "hdr_bits": int(t[317]), "btype": int(t[318]), "dist_len": int(t[319]), "dist_code": int(t[320])})
    return out


def sequential_sum(x) -> float:
    """fp32 left-to-right sum with per-step rounding (CMatrix::avg's arithmetic), evaluated by the exact parallel scan."""
    torch = _torch()
    _chk_f32(x, "x")
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _check(lib().fav_sequential_sum_f32(_p(x), C.c_size_t(x.numel()), _p(out), _stream()))
    return out


def temporal_loss(prev_rgb, cur_rgb, backward_flo, cert_u8, border: int = BORDER_STN) -> float:
    """fast_artistic_video.lua:128-151: MSE between the flow-warped previous and the current stylised frame on reliable pixels."""
    _chk_f32(prev_rgb, "prev_rgb"); _chk_f32(cur_rgb, "cur_rgb")
    _, h, w = prev_rgb.shape
    out = C.c_double()
    _check(lib().fav_temporal_loss_host(_p(prev_rgb), _p(cur_rgb), _p(backward_flo), _p(cert_u8), h, w, border, C.byref(out), _stream()))
    return out.value


class _VROpts(C.Structure):
    _fields_ = [("overlap_w", C.c_int), ("overlap_h", C.c_int), ("occlusions_min_filter", C.c_int), ("median_filter", C.c_int),
                ("fill_random", C.c_int), ("seed", C.c_uint), ("create_inconsistent", C.c_int),
                ("create_inconsistent_border", C.c_int), ("out_equi_w", C.c_int), ("out_equi_h", C.c_int), ("border_mode", C.c_int)]


def vr_map_host(kind: int, hplus: int, wplus: int, overlap: int, median: int = 3, out_w: int = 0, out_h: int = 0) -> np.ndarray:
    """Static maps of the cube-map orchestration (vr_helper.lua), computed on the host: no device needed."""
    shape = (2, out_h, out_w) if kind == 4 else (2, hplus, wplus)
    out = np.empty(shape, np.float32)
    _check(lib().fav_vr_map_host(kind, hplus, wplus, overlap, median, out_w, out_h, out.ctypes.data_as(C.c_void_p)))
    return out


def vr_equi_to_faces(equi_u8_hwc, edge: int, overlap_w: int, overlap_h: Optional[int] = None, supersample: int = 2, want_f32: bool = False):
    """fav_vr_equi_to_faces_rgb8: one equirectangular frame (u8 [H][W][3]) -> the six expanded cube faces in processing order, a list of
    u8 [edge][edge][3] tensors; with want_f32 also the list of the unrounded fp32 planes [edge][edge][3] (0..255 units)."""
    torch = _torch()
    if not (equi_u8_hwc.is_cuda and equi_u8_hwc.dtype == torch.uint8 and equi_u8_hwc.is_contiguous() and equi_u8_hwc.dim() == 3 and
            equi_u8_hwc.shape[2] == 3):
        raise FavError("vr_equi_to_faces: the frame must be a contiguous uint8 CUDA tensor [H][W][3]")
    overlap_h = overlap_w if overlap_h is None else overlap_h
    eh, ew = equi_u8_hwc.shape[0], equi_u8_hwc.shape[1]
    faces = [torch.empty((edge, edge, 3), dtype=torch.uint8, device=equi_u8_hwc.device) for _ in range(6)]
    planes = [torch.empty((edge, edge, 3), dtype=torch.float32, device=equi_u8_hwc.device) for _ in range(6)] if want_f32 else None
    arr = lambda ts: (C.c_void_p * 6)(*[t.data_ptr() for t in ts])
    _check(lib().fav_vr_equi_to_faces_rgb8(_p(equi_u8_hwc), ew, eh, edge, edge, overlap_w, overlap_h, supersample, arr(faces),
                                           arr(planes) if want_f32 else None, _stream()))
    return (faces, planes) if want_f32 else faces


class VR:
    """360-degree cube-map orchestration (fast_artistic_video_vr.lua): six faces per frame, see include/fav.h."""

    def __init__(self, net: Net, hplus: int, wplus: int, overlap_w: int = 20, overlap_h: int = 20, min_filter_r: int = 7,
                 median: int = 3, out_equi_w: int = 0, out_equi_h: int = 0, fill_random: bool = False, seed: int = 1,
                 image_net: Optional[Net] = None, create_inconsistent: bool = False, create_inconsistent_border: bool = False,
                 border: int = BORDER_STN):
        self.net, self.img, self.H, self.W = net, image_net, hplus, wplus
        o = _VROpts(overlap_w, overlap_h, min_filter_r, median, int(fill_random), seed, int(create_inconsistent),
                    int(create_inconsistent_border), out_equi_w, out_equi_h, border)
        hd = C.c_void_p()
        _check(lib().fav_vr_create(net.h, image_net.h if image_net is not None else None, hplus, wplus, C.byref(o), C.byref(hd)))
        self.h = hd
        net._retain()
        if image_net is not None:
            image_net._retain()
        sz = [C.c_int() for _ in range(6)]
        _check(lib().fav_vr_output_sizes(self.h, *[C.byref(x) for x in sz]))
        self.equi_w, self.equi_h, self.cube_w, self.cube_h, self.filt_w, self.filt_h = [x.value for x in sz]

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            try:
                lib().fav_vr_destroy(self.h)
            except Exception:      # interpreter shutdown
                pass
            self.h = None
            self.net._release()
            if self.img is not None:
                self.img._release()

    __del__ = close

    def face(self, i: int, frame_u8_hwc, backward_flo=None, cert_u8=None):
        torch = _torch()
        out = torch.empty((3, self.H, self.W), dtype=torch.float32, device=frame_u8_hwc.device)
        _check(lib().fav_vr_face(self.h, i, _p(frame_u8_hwc), _p(backward_flo), _p(cert_u8), _p(out), _stream()))
        return out

    def face_flow(self, i: int, frame_u8_hwc, backward_flo=None, forward_flo=None, use_structure=False):
        """fav_vr_face_flow: the face with the consistency check made on the device from the two flows (no certainty file)"""
        torch = _torch()
        out = torch.empty((3, self.H, self.W), dtype=torch.float32, device=frame_u8_hwc.device)
        _check(lib().fav_vr_face_flow(self.h, i, _p(frame_u8_hwc), _p(backward_flo), _p(forward_flo), 1 if use_structure else 0,
                                      _p(out), _stream()))
        return out

    def prefetch_mask(self, i: int, frame_u8_hwc, backward_flo=None, forward_flo=None, use_structure=False):
        """fav_vr_prefetch_mask: start face i's mask on the VR object's side stream; the matching face_flow consumes it"""
        _check(lib().fav_vr_prefetch_mask(self.h, i, _p(frame_u8_hwc), _p(backward_flo), _p(forward_flo), 1 if use_structure else 0,
                                          _stream()))

    def last_mask(self):
        """copy of the u8 mask the last face_flow computed (before the border max and the min filter)"""
        torch = _torch()
        ptr = lib().fav_vr_last_mask(self.h)
        if not ptr:
            raise FavError("fav_vr_last_mask: no face has been checked on the device yet")
        out = torch.empty((self.H, self.W), dtype=torch.uint8, device=f"cuda:{self.net.device}")
        out.view(-1).copy_(_from_ptr_u8(ptr, self.H * self.W, self.net.device))
        return out

    def finish_frame(self, want_equi: bool = True, want_cube: bool = True):
        torch = _torch()
        dev = torch.device("cuda", torch.cuda.current_device())
        e = torch.empty((self.equi_h, self.equi_w, 3), dtype=torch.uint8, device=dev) if (want_equi and self.equi_w) else None
        c = torch.empty((self.cube_h, self.cube_w, 3), dtype=torch.uint8, device=dev) if (want_cube and self.cube_w) else None
        _check(lib().fav_vr_finish_frame(self.h, _p(e), _p(c), _stream()))
        return e, c

    def get(self, which: int, k: int = 0, out=None):
        """fav_vr_get_f32 into a new tensor, or into `out` (a contiguous float32 CUDA tensor of the kind's shape; a refusal leaves it as
        it was)"""
        torch = _torch()
        shape = {0: (3, self.H, self.W), 1: (3, self.H, self.W), 2: (3, self.filt_h, self.filt_w),
                 3: (3, self.equi_h, self.equi_w), 4: (3, self.cube_h, self.cube_w), 5: (self.H, self.W),
                 6: (3, self.H, self.W), 7: (3, self.H, self.W)}[which]       # 6: the last face's border sum, 7: its prior
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
            raise FavError(f"VR.get: out must be a contiguous float32 CUDA tensor {list(shape)}")
        _check(lib().fav_vr_get_f32(self.h, which, k, _p(out), _stream()))
        return out

    def last_padded_input(self, out=None):
        """fav_vr_get_padded_input_f32: [H + 2p][W + 2p][8] network input of the last face as the network read it (p = Net.input_pad,
        eighth channel zero), copied device to device"""
        torch = _torch()
        p = self.net.input_pad()
        shape = (self.H + 2 * p, self.W + 2 * p, 8)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=f"cuda:{self.net.device}")
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape):
            raise FavError(f"VR.last_padded_input: out must be a contiguous float32 CUDA tensor {list(shape)}")
        _check(lib().fav_vr_get_padded_input_f32(self.h, _p(out), _stream()))
        return out

    def set(self, which: int, k: int, tensor):
        """fav_vr_set_f32: write raw face k of this frame (which = 0; six of them and finish_frame runs) or blended face k of the finished
        frame (which = 1; six of them make a previous frame) from a contiguous f32 CUDA tensor [3][hplus][wplus]"""
        torch = _torch()
        if tensor is not None and not (tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous() and
                                       tuple(tensor.shape) == (3, self.H, self.W)):
            raise FavError(f"VR.set: the face must be a contiguous float32 CUDA tensor [3][{self.H}][{self.W}]")
        _check(lib().fav_vr_set_f32(self.h, which, k, _p(tensor), _stream()))


def _from_ptr_u8(ptr: int, n: int, device: int):
    """wrap a raw device pointer as a torch uint8 tensor (no ownership) via __cuda_array_interface__"""
    torch = _torch()

    class _W:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(_W(), device=f"cuda:{device}")


# ------------------------------------------------------------------------------------------------ host formats
def read_flo(path: str) -> np.ndarray:
    d = C.POINTER(C.c_float)(); w, h = C.c_int(), C.c_int()
    _check(lib().fav_read_flo_host(path.encode(), C.byref(d), C.byref(w), C.byref(h)))
    try:
        return np.ctypeslib.as_array(d, shape=(h.value, w.value, 2)).copy()
    finally:
        lib().fav_free_host(d)


def read_pnm(path: str) -> np.ndarray:
    d = C.POINTER(C.c_uint8)(); w, h, ch = C.c_int(), C.c_int(), C.c_int()
    _check(lib().fav_read_pnm_host(path.encode(), C.byref(d), C.byref(w), C.byref(h), C.byref(ch)))
    try:
        a = np.ctypeslib.as_array(d, shape=(h.value, w.value, ch.value)).copy()
        return a if ch.value == 3 else a[..., 0]
    finally:
        lib().fav_free_host(d)


def write_pgm(path: str, a: np.ndarray) -> None:
    a = np.ascontiguousarray(a, np.uint8)
    _check(lib().fav_write_pgm_host(path.encode(), a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]))


def write_png(path: str, rgb_hwc: np.ndarray, level: int = 1) -> None:
    a = np.ascontiguousarray(rgb_hwc, np.uint8)
    _check(lib().fav_write_png_rgb8_host(path.encode(), a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], level))
