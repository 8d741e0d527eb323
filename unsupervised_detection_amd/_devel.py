"""Loader of libudet_debug.so (include/udet_debug.h): TEST-ONLY hooks that pin a convolution kernel family / tile / split-K
mode and report which one ran.  Used by tests/ and tools/ only -- nothing on the product path imports this module; the
hooks are not exported by libudet.so."""
from __future__ import annotations

import ctypes
import os

from ._ffi import check as _check, lib as _lib  # libudet.so first: the debug library resolves its internal symbols against it  # noqa: F401

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libudet_debug.so")
if not os.path.exists(_PATH):
    raise RuntimeError(f"{_PATH} is missing: build it with `make -C unsupervised_detection_amd/csrc`")
dbg = ctypes.CDLL(_PATH, mode=ctypes.RTLD_GLOBAL)
dbg.udet_debug_force_conv.restype = None
dbg.udet_debug_force_conv.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
dbg.udet_debug_last_conv.restype = ctypes.c_int
dbg.udet_debug_last_conv.argtypes = []
dbg.udet_debug_conv_fp16.restype = None
dbg.udet_debug_conv_fp16.argtypes = [ctypes.c_int]
dbg.udet_debug_conv_fp16_grad_scale.restype = None
dbg.udet_debug_conv_fp16_grad_scale.argtypes = [ctypes.c_float]
dbg.udet_debug_force_wgrad.restype = None
dbg.udet_debug_force_wgrad.argtypes = [ctypes.c_int, ctypes.c_int]
dbg.udet_debug_upb_min_pixels.restype = None
dbg.udet_debug_upb_min_pixels.argtypes = [ctypes.c_long]
dbg.udet_debug_set_tuning.restype = None
dbg.udet_debug_set_tuning.argtypes = [ctypes.c_int]
dbg.udet_debug_last_wgrad.restype = ctypes.c_int
dbg.udet_debug_last_wgrad.argtypes = []
dbg.udet_debug_force_pair.restype = None
dbg.udet_debug_force_pair.argtypes = [ctypes.c_int]
dbg.udet_debug_last_pair.restype = ctypes.c_int
dbg.udet_debug_last_pair.argtypes = []
dbg.udet_debug_conv2d_pair.restype = ctypes.c_int
dbg.udet_debug_conv2d_pair.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_int] * 10 + [ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
dbg.udet_debug_last_wgrad_reduce.restype = ctypes.c_int
dbg.udet_debug_last_wgrad_reduce.argtypes = []
_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
dbg.udet_debug_conv2d_backward_filter_ex.restype = ctypes.c_int
dbg.udet_debug_conv2d_backward_filter_ex.argtypes = ([_p, _i, _i, _p, _i, _i, _p, _i, _f, _p, _p, _p, _f, _p, _p, _p, _p] + [_i] * 9
                                                     + [_p, ctypes.c_size_t, _p])
# one level of the recover decoder's low-resolution form as a plan runs it (include/udet_debug.h)
UPCONV_WSETS_OFFSET = 6400  # UDET_DEBUG_UPCONV_WSETS_OFFSET: floats in front of the packed weight sets in the entries' workspace
dbg.udet_debug_upconv_lowres_workspace_bytes.restype = ctypes.c_size_t
dbg.udet_debug_upconv_lowres_workspace_bytes.argtypes = [_i, _i, _i]
dbg.udet_debug_upconv_lowres_fwd.restype = ctypes.c_int
dbg.udet_debug_upconv_lowres_fwd.argtypes = [_p, _i, _p, _p, _i, _f, _p, _i, _i, _p] + [_i] * 6 + [_p, ctypes.c_size_t, _p]
dbg.udet_debug_upconv_lowres_bwd.restype = ctypes.c_int
dbg.udet_debug_upconv_lowres_bwd.argtypes = [_p, _i, _i, _p, _p, _i, _p] + [_i] * 5 + [_p, ctypes.c_size_t, _p]
dbg.udet_debug_upconv_tables.restype = ctypes.c_int
dbg.udet_debug_upconv_tables.argtypes = [_i, _i, _i] + [_p] * 4 + [_i, _p]
dbg.udet_debug_max_segs.restype = ctypes.c_int
dbg.udet_debug_max_segs.argtypes = []
# the glue launchers of csrc/elementwise.hip, one launch each (include/udet_debug.h; tests/test_glue_gpu.py)
_l = ctypes.c_long
for _name, _args in (("resize_bilinear_fwd", [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _i, _f, _f, _p]),
                     ("resize_bilinear_bwd", [_p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p]),
                     ("share_samples", [_p, _l, _i, _i, _i, _i, _p]),
                     ("fold_samples", [_p, _l, _i, _i, _i, _i, _p]),
                     ("emit_du", [_p, _p, _p, _l, _i, _i, _i, _i, _f, _p]),
                     ("pack_pwc_input", [_p, _p, _p, _l, _p]),
                     ("gen_input", [_p, _p, _p, _i, _l, _p, ctypes.c_size_t, _p]),
                     ("mask_rec_inputs", [_p, _p, _p, _p, _l, _i, _p]),
                     ("pack_imgin", [_p, _p, _l, _i, _p]),
                     ("mask_bwd", [_p, _p, _p, _p, _p, _l, _p])):
    _fn = getattr(dbg, "udet_debug_launch_" + _name)
    _fn.restype = ctypes.c_int
    _fn.argtypes = _args
dbg.udet_debug_gen_input_workspace_bytes.restype = ctypes.c_size_t
dbg.udet_debug_gen_input_workspace_bytes.argtypes = [_i]


class ConvEx(ctypes.Structure):
    """udet_debug_conv_ex (include/udet_debug.h): one convolution launch as a step plan builds it; unset fields are 0 / NULL."""
    _fields_ = ([("form", _i)] + [(k, _i) for k in ("n", "h", "wd", "cin", "cout", "k", "stride", "dilation", "up", "kc", "k_split", "k_gap")]
                + [("x", _p), ("ldx", _i), ("x_coff", _i), ("xa", _p), ("xact", _i), ("xalpha", _f), ("w", _p), ("bias", _p), ("act", _i),
                   ("alpha", _f), ("y", _p), ("ldy", _i), ("y_coff", _i), ("res", _p), ("ldres", _i), ("res_coff", _i), ("y2", _p),
                   ("ldy2", _i), ("y2_coff", _i), ("accumulate", _i), ("uo", _p), ("ldu", _i), ("u_coff", _i), ("ua", _p), ("ldua", _i),
                   ("ua_coff", _i), ("uact", _i), ("ualpha", _f), ("u_c0", _i), ("u_c1", _i), ("pack_job", _i)])


dbg.udet_debug_conv2d_ex_workspace_bytes.restype = ctypes.c_size_t
dbg.udet_debug_conv2d_ex_workspace_bytes.argtypes = [ctypes.POINTER(ConvEx)]
dbg.udet_debug_conv2d_ex.restype = ctypes.c_int
dbg.udet_debug_conv2d_ex.argtypes = [ctypes.POINTER(ConvEx), _p, ctypes.c_size_t, _p]


dbg.udet_debug_conv2d_pair_ex_workspace_bytes.restype = ctypes.c_size_t
dbg.udet_debug_conv2d_pair_ex_workspace_bytes.argtypes = [ctypes.POINTER(ConvEx), ctypes.POINTER(ConvEx)]
dbg.udet_debug_conv2d_pair_ex.restype = ctypes.c_int
dbg.udet_debug_conv2d_pair_ex.argtypes = [ctypes.POINTER(ConvEx), ctypes.POINTER(ConvEx), _p, ctypes.c_size_t, _p]


class HeadEx(ctypes.Structure):
    """udet_debug_head_ex (include/udet_debug.h): a 2-channel head in the GEMM + gather form as a plan runs it; unset fields are 0 / NULL."""
    _fields_ = ([(k, _i) for k in ("n", "h", "wd", "cin", "k", "kc", "k_split", "k_gap")]
                + [("x", _p), ("ldx", _i), ("x_coff", _i), ("w", _p), ("bias", _p), ("y", _p), ("ldy", _i), ("y_coff", _i), ("transposed", _i),
                   ("pack_job", _i)])


dbg.udet_debug_conv2d_head_ex_workspace_bytes.restype = ctypes.c_size_t
dbg.udet_debug_conv2d_head_ex_workspace_bytes.argtypes = [ctypes.POINTER(HeadEx)]
dbg.udet_debug_conv2d_head_ex.restype = ctypes.c_int
dbg.udet_debug_conv2d_head_ex.argtypes = [ctypes.POINTER(HeadEx), _p, ctypes.c_size_t, _p]
dbg.udet_debug_warp_cost_volume_ex.restype = ctypes.c_int
dbg.udet_debug_warp_cost_volume_ex.argtypes = [_p, _p, _p, _i, _i, _f, _p, _i, _i, _i, _i, _i, _i, _i, _p]


def _workspace_and_stream(workspace, stream):
    if workspace is None or isinstance(workspace, tuple):
        ptr, nbytes = workspace or (None, 0)
    else:
        ptr, nbytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
    return ptr, nbytes, stream


def conv2d_pair_ex(a_fields, b_fields, workspace=None, stream=None):
    """udet_debug_conv2d_pair_ex: two problems, each a dict of the struct's fields as conv2d_ex takes them (None: a NULL struct), through
    the pair launcher; workspace: a float32 device tensor of conv2d_pair_ex_workspace_bytes(a_fields, b_fields) bytes, or (pointer, bytes)."""
    a, b = (None if f is None else ctypes.byref(conv_ex_args(**f)) for f in (a_fields, b_fields))
    _check(dbg.udet_debug_conv2d_pair_ex(a, b, *_workspace_and_stream(workspace, stream)))


def conv2d_pair_ex_workspace_bytes(a_fields, b_fields) -> int:
    a, b = (None if f is None else ctypes.byref(conv_ex_args(**f)) for f in (a_fields, b_fields))
    return int(dbg.udet_debug_conv2d_pair_ex_workspace_bytes(a, b))


def conv2d_ex(workspace=None, stream=None, **fields):
    """udet_debug_conv2d_ex with the struct's fields as keywords (tensors: their data pointers, or (tensor, element offset) for a pointer into
    one); workspace: a float32 device tensor of conv2d_ex_workspace_bytes(**fields) bytes, or (pointer, bytes).  A refusal raises
    ValueError (_ffi.check) before anything reaches the device; a pointer given as a plain int is passed as it is."""
    a = conv_ex_args(**fields)
    _check(dbg.udet_debug_conv2d_ex(ctypes.byref(a), *_workspace_and_stream(workspace, stream)))


def conv_ex_args(**fields) -> ConvEx:
    a = ConvEx()
    for k, v in fields.items():
        if isinstance(v, tuple):
            v = v[0].data_ptr() + v[1] * v[0].element_size()
        elif hasattr(v, "data_ptr"):
            v = v.data_ptr()
        setattr(a, k, v)
    return a


def conv2d_ex_workspace_bytes(**fields) -> int:
    return int(dbg.udet_debug_conv2d_ex_workspace_bytes(ctypes.byref(conv_ex_args(**fields))))


def _pointer(v):
    if isinstance(v, tuple):
        return v[0].data_ptr() + v[1] * v[0].element_size()
    return v.data_ptr() if hasattr(v, "data_ptr") else v


def head_ex_args(**fields) -> HeadEx:
    a = HeadEx()
    for k, v in fields.items():
        setattr(a, k, _pointer(v))
    return a


def conv2d_head_ex_workspace_bytes(**fields) -> int:
    return int(dbg.udet_debug_conv2d_head_ex_workspace_bytes(ctypes.byref(head_ex_args(**fields))))


def conv2d_head_ex(workspace=None, stream=None, **fields):
    """udet_debug_conv2d_head_ex with the struct's fields as keywords (tensors, (tensor, element offset) or plain integers for the pointers, as
    conv2d_ex takes them); workspace: a float32 device tensor of conv2d_head_ex_workspace_bytes(**fields) bytes, or (pointer, bytes)."""
    a = head_ex_args(**fields)
    _check(dbg.udet_debug_conv2d_head_ex(ctypes.byref(a), *_workspace_and_stream(workspace, stream)))


def warp_cost_volume_ex(c1, c2, flow, ldf, f_coff, flow_scale, out, ldo, corr_coff, c1_coff, n, h, w, c, stream=None):
    """udet_debug_warp_cost_volume_ex on the current stream: launch_warp_cost_volume with a plan's slab arguments (flow None: level 6; pointers
    as tensors, (tensor, element offset) or plain integers); a refusal raises ValueError (_ffi.check) before anything reaches the device."""
    _, _, stream = _workspace_and_stream(None, stream)
    _check(dbg.udet_debug_warp_cost_volume_ex(_pointer(c1), _pointer(c2), None if flow is None else _pointer(flow), ldf, f_coff, flow_scale,
                                              _pointer(out), ldo, corr_coff, c1_coff, n, h, w, c, stream))


def launch(name: str, *args):
    """udet_debug_launch_<name>(*args, current stream) with tensors passed as their data pointers; a refusal raises ValueError
    (_ffi.check) before anything reaches the device."""
    import torch
    raw = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    _check(getattr(dbg, "udet_debug_launch_" + name)(*raw, torch.cuda.current_stream().cuda_stream))


def upconv_tables(h: int, w: int, backward: bool):
    """The segment and tap tables of the recover decoder's low-resolution form for an h x w source (host only, no device needed):
    dict(nseg, seg [nseg][oy, ox, h, w], seg_tap [nseg + 1], taps [ntaps][dy, dx, widx]); a refusal raises ValueError (_ffi.check)."""
    cap = 1024
    nseg, ntaps = ctypes.c_int(0), ctypes.c_int(0)
    seg, seg_tap, taps = (ctypes.c_int * 64)(), (ctypes.c_int * 17)(), (ctypes.c_int * (3 * cap))()
    st = dbg.udet_debug_upconv_tables(h, w, 1 if backward else 0, ctypes.addressof(nseg), ctypes.addressof(seg), ctypes.addressof(seg_tap),
                                      ctypes.addressof(taps), cap, ctypes.addressof(ntaps))
    _check(st)
    ns, nt = nseg.value, ntaps.value
    return dict(nseg=ns, seg=[tuple(seg[4 * s:4 * s + 4]) for s in range(ns)], seg_tap=list(seg_tap[:ns + 1]),
                taps=[tuple(taps[3 * t:3 * t + 3]) for t in range(nt)])
