"""Native-resolution stage, beside step 4: the displacements the motion-compensated link reads (csrc/motion.hip).

  flow_displacements(flow, layout)              one call of udet_flow_displacements_ragged: a batch of flow fields of one size -> one
                                                packed int32 (dx low, dy high 16 bits) per pixel of the batch's native-size frames --
                                                the `disp` of native_tracks.link_detections
  check_flow_arguments                          its host validation (no GPU needed)
  BackwardFlow                                  the driver's default provider of those flow fields: the PWC flow from every frame of a
                                                batch to the frame before it, at one fixed size
  motion_params / motion_size                   the `motion` dict of native_tracks.track_params, filled in and checked"""
import torch

from ._ffi import check, lib
from .ragged import PackedLayout, as_layout, require_tensor

MOTION_DEFAULTS = {"size": (384, 640)}
FLOW_MAX = 32767  # the largest flow grid side: a tap index and a displacement fit 16 bits


def motion_size(size):
    """(fh, fw) as the flow network takes it: a pair of positive multiples of 64 (ValueError otherwise; bools and floats are refused)."""
    try:
        fh, fw = size
    except (TypeError, ValueError):
        raise ValueError("tracks: motion size must be a pair (fh, fw)")
    for v in (fh, fw):
        if isinstance(v, bool) or not isinstance(v, int) or v < 64 or v % 64 or v > FLOW_MAX:
            raise ValueError("tracks: motion size must be a pair of positive multiples of 64 (at most {})".format(FLOW_MAX))
    return int(fh), int(fw)


def motion_params(motion=None):
    """The `motion` dict of the `tracks` dict ({} or None: the defaults) with the defaults filled in and checked (ValueError)."""
    p = dict(MOTION_DEFAULTS)
    if motion is not None:
        if not isinstance(motion, dict) or not set(motion) <= set(MOTION_DEFAULTS):
            raise ValueError("tracks: motion must be a dict with keys among {}".format(sorted(MOTION_DEFAULTS)))
        p.update({k: v for k, v in motion.items() if v is not None})
    p["size"] = motion_size(tuple(p["size"]) if isinstance(p["size"], list) else p["size"])
    return p


def check_flow_arguments(flow, layout):
    """The host validation of flow_displacements (ValueError): flow is a float32 tensor [n, fh, fw, 2] with fh, fw in 1..32767 and
    layout a PackedLayout (or an object that carries one as .layout) of n one-channel samples, at most 65535.  Returns (layout, fh, fw)."""
    layout = getattr(layout, "layout", layout)
    if not isinstance(layout, PackedLayout):
        raise ValueError("layout must be the PackedLayout of the frames the displacements are for (or an object with one as .layout)")
    as_layout(layout, None, layout.numel, max_samples=65535)
    require_tensor(flow, "flow (one (u, v) field per frame)", torch.float32, 4, cuda=False)
    n, fh, fw, two = (int(v) for v in flow.shape)
    if n != layout.n or two != 2:
        raise ValueError("flow must be [n, fh, fw, 2] with one field per frame of the layout ({} frames)".format(layout.n))
    if not (1 <= fh <= FLOW_MAX and 1 <= fw <= FLOW_MAX):
        raise ValueError("flow: a grid of fh x fw with both in 1..{} is required".format(FLOW_MAX))
    return layout, fh, fw


def flow_displacements(flow, layout) -> torch.Tensor:
    """One packed integer displacement per pixel of a ragged batch of native-size frames, in one launch of
    udet_flow_displacements_ragged.  flow: device float32 [n, fh, fw, 2], (u, v) in flow-grid pixels, row i from frame i to the frame
    before it (PWCFlow's convention); layout: the PackedLayout of the n frames' labels (or the ComponentSelection / Detections that
    carries it).  Per pixel the field is sampled bilinearly at the pixel's centre, scaled to native pixels (W / fw, H / fh), rounded to
    the nearest integer (ties to even) and packed: dx in the low 16 bits, dy in the high 16, both signed -- float32 arithmetic fixed
    operation by operation in include/udet.h, so the result is the same numbers wherever it is computed.  Returns int32 [total] on
    flow's device: the `disp` of link_detections.  Validated on the host before the device is touched (ValueError)."""
    layout, fh, fw = check_flow_arguments(flow, layout)
    require_tensor(flow, "flow (one (u, v) field per frame)", torch.float32, 4)
    dev = flow.device
    d_off, d_hw = layout.device_tables(dev)
    disp = torch.empty(layout.numel, dtype=torch.int32, device=dev)
    check(lib.udet_flow_displacements_ragged(flow.data_ptr(), layout.n, fh, fw, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h, layout.max_w,
                                             layout.numel, disp.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return disp


class BackwardFlow(object):
    """The flow from every frame of a batch to the frame before it, at one fixed size: the driver's default `motion_flow`.
    flow_fn: a post_processing.PWCFlow (None: one is built on first use, as post_process builds its own); size = (fh, fw), both
    multiples of 64; flow_batch: pairs per network call.  provider(frames) takes the batch's native frames (the ragged uint8 frames
    load_images_device returns), resizes them to `size` (data.crop_flip_resize_ragged) and returns device float32 [n, fh, fw, 2]: row i
    = flow_fn(frame i, frame i - 1), row 0 against the last resized frame of the call before -- zeros without one (that row is never
    read: such a frame starts a sequence).  It keeps the batch's last resized frame for the next call; reset() forgets it (between
    categories)."""

    def __init__(self, flow_fn=None, size=(384, 640), flow_batch=8):
        self.size = motion_size(tuple(size) if isinstance(size, list) else size)
        if isinstance(flow_batch, bool) or not isinstance(flow_batch, int) or flow_batch < 1:
            raise ValueError("flow_batch must be an int of at least 1")
        self.flow_fn, self.flow_batch, self.prev = flow_fn, flow_batch, None

    def reset(self):
        self.prev = None

    def __call__(self, frames):
        from .data import crop_flip_resize_ragged
        if self.flow_fn is None:
            from .post_processing import PWCFlow
            self.flow_fn = PWCFlow()
        fh, fw = self.size
        small = crop_flip_resize_ragged(frames.data, frames.layout, None, 3, fh, fw)  # float32 [n, fh, fw, 3] in 0..255
        n = int(small.shape[0])
        first = 0 if self.prev is not None else 1
        flow = torch.zeros((n, fh, fw, 2), dtype=torch.float32, device=small.device)
        if n > first:
            before = ([self.prev] if first == 0 else []) + [small[i - 1] for i in range(1, n)]
            flow[first:] = self.flow_fn.batch([small[i] for i in range(first, n)], before, batch=self.flow_batch)
        self.prev = small[n - 1].clone()
        return flow
