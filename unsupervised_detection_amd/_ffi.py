"""ctypes binding of libudet.so (include/udet.h).

The HIP library is the product: there is no CPU / PyTorch fallback.  Importing this
module without a built ``libudet.so`` raises, and every call that fails raises with
``udet_last_error()``.
"""
from __future__ import annotations

import ctypes
import os

# PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so); libudet.so names the runtime by soname.  Loaded AFTER torch the
# library binds to the runtime torch already initialised; loaded first it would bring /opt/rocm's copy in, torch would add its own, and
# whichever initialises second sees "no ROCm-capable device".  Hence: torch first, always.
import torch  # noqa: F401  (load order, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libudet.so")

if not os.path.exists(LIB_PATH):
    raise RuntimeError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(or `make -C unsupervised_detection_amd/csrc`).  There is no CPU fallback.")

lib = ctypes.CDLL(LIB_PATH)

c_f = ctypes.c_float
c_i = ctypes.c_int
c_p = ctypes.c_void_p
c_sz = ctypes.c_size_t

lib.udet_version.restype = c_i
lib.udet_last_error.restype = ctypes.c_char_p


def sig(name, restype, *argtypes):
    """Declare the C signature of lib.<name>; returns the function."""
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


sig("udet_warp", c_i, c_p, c_p, c_f, c_p, c_i, c_i, c_i, c_i, c_p)
sig("udet_warp_debug", c_i, c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p)
sig("udet_cost_volume", c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p)
sig("udet_resize_bilinear_legacy_fwd", c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p)
sig("udet_resize_bilinear_legacy_bwd", c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p)
sig("udet_conv2d_workspace_bytes", c_sz, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i)
sig("udet_conv2d", c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_sz, c_p)
sig("udet_conv2d_backward_data", c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p,
     c_sz, c_p)
sig("udet_conv2d_backward_filter", c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i,
     c_f, c_p, c_sz, c_p)
sig("udet_conv2d_transpose4x4s2", c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_sz, c_p)


sig("udet_warp_cost_volume", c_i, c_p, c_p, c_p, c_f, c_p, c_p, c_i, c_i, c_i, c_i, c_p)
sig("udet_stage_workspace_bytes", c_sz, c_i)
sig("udet_flow_normalize", c_i, c_p, c_p, c_i, c_i, c_i, c_p, c_sz, c_p)
sig("udet_charbonnier_loss", c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_sz, c_p)
sig("udet_losses_forward", c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_p, c_p, c_p, c_sz, c_p)
sig("udet_losses_backward", c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p, c_p, c_p)
sig("udet_clip_or_noise", c_i, c_p, c_sz, c_f, c_p, ctypes.c_ulonglong, ctypes.c_long, c_p)
sig("udet_adam_step", c_i, c_p, c_p, c_p, c_p, c_sz, c_f, c_f, c_f, c_f, ctypes.c_long, c_p)
sig("udet_generator_layers", c_i, c_p, c_p, c_p)
sig("udet_generator_backward", c_i, c_p, c_p, c_p, c_p, c_p)
sig("udet_recover_backward", c_i, c_p, c_p, c_p, c_p, c_p)
sig("udet_grad_absmean", c_i, c_p, c_i, c_p, c_p, c_p, c_p)
sig("udet_stream_wait_grads", c_i, c_p, c_i, c_p)
sig("udet_tune_rejected", c_i)
sig("udet_tune_save", c_i, ctypes.c_char_p)
sig("udet_tune_load", c_i, ctypes.c_char_p)
# visualisation and training summaries (visualize.py)
sig("udet_flow_to_image_workspace_bytes", c_sz, c_i)
sig("udet_flow_to_image", c_i, c_p, c_p, c_p, c_f, c_i, c_i, c_i, c_p, c_p, c_sz, c_p)
sig("udet_overlay_mask", c_i, c_p, c_p, c_p, c_f, c_i, c_i, c_i, c_p, c_i, c_i, c_p)
sig("udet_overlay_native_ragged", c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_f, c_f, ctypes.c_uint, c_i, ctypes.c_uint, c_p, c_p)
# detections at native size (native_results.component_boxes, visualize.draw_boxes)
sig("udet_component_boxes_workspace_bytes", c_sz, c_sz, c_i, c_i)
sig("udet_component_boxes_ragged", c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_i, c_i, c_p, c_p, c_p, c_sz, c_p)
sig("udet_draw_boxes_ragged", c_i, c_p, c_i, c_p, c_p, c_sz, c_p, c_p, c_i, c_i, ctypes.c_uint, c_p)
# detections linked into tracks (native_results.link_detections, visualize.draw_track_boxes)
sig("udet_link_detections_workspace_bytes", c_sz, c_sz, c_i, c_i, c_i, c_i)
sig("udet_link_detections_ragged", c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i,
    c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p)
sig("udet_link_detections_gap_workspace_bytes", c_sz, c_sz, c_i, c_i, c_i, c_i, c_i, c_i)
sig("udet_link_detections_gap_ragged", c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_p, c_p, c_i, c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p,
    c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p)
# motion-compensated linking (native_motion.flow_displacements, native_tracks.link_detections(disp=...)): disp before the workspace
sig("udet_flow_displacements_ragged", c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_sz, c_p, c_p)
sig("udet_link_detections_motion_ragged", c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i,
    c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p)
sig("udet_link_detections_gap_motion_ragged", c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_p, c_p, c_i, c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p,
    c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p)
sig("udet_draw_track_boxes_ragged", c_i, c_p, c_i, c_p, c_p, c_sz, c_p, c_p, c_i, c_p, c_i, c_p, c_i, c_p)
# per-track instance maps and their picture (native_instances.instance_maps, visualize.overlay_instances)
sig("udet_track_instance_maps_workspace_bytes", c_sz, c_sz, c_i, c_i)
sig("udet_track_instance_maps_ragged", c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p)
sig("udet_overlay_instances_ragged", c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_f, c_f, c_p, c_i, ctypes.c_uint, c_i, c_p, c_p)
# the masks of whole tracks (native_follow.follow_tracks)
sig("udet_follow_tracks_workspace_bytes", c_sz, c_sz, c_i, c_i)
sig("udet_follow_tracks_ragged", c_i, c_p, c_i, c_p, c_p, c_i, c_i, ctypes.c_longlong, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p)
# tracks against multi-object annotations (native_objects.object_overlaps)
sig("udet_track_object_overlaps_workspace_bytes", c_sz, c_sz, c_i, c_i)
sig("udet_track_object_overlaps_ragged", c_i, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_p, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_sz, c_p)
sig("udet_histogram_limits", c_i, c_p, c_i)
sig("udet_grad_histogram_workspace_bytes", c_sz, c_i)
sig("udet_grad_histogram", c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_sz, c_p)


class UdetError(RuntimeError):
    pass


class UdetOverflow(OverflowError):
    """UDET_ERR_OVERFLOW (-6): an fp16-mode optimizer update was dropped on the device (include/udet.h, udet_config.conv_fp16).
    Its own type, so that callers which retry on it (trainer.train_step) do not swallow Python's / ctypes' own OverflowError
    (argument marshalling of a too-large integer, for example)."""


def check(status: int):
    if status != 0:
        msg = lib.udet_last_error().decode("utf-8", "replace")
        if status in (-1, -2, -5):
            raise ValueError(f"libudet error {status}: {msg}")
        if status == -6:
            raise UdetOverflow(f"libudet error {status}: {msg}")
        raise UdetError(f"libudet error {status}: {msg}")
