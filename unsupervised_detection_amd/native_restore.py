"""Native-resolution stage, step 1: a batch of masks restored to each frame's own size (csrc/restore.hip).

Every mask the networks produce is img_height x img_width (192 x 384) and covers the central test_crop (0.9) of the frame; the
benchmarks (DAVIS-2016, FBMS-59, SegTrackV2) are scored on the full frame at each frame's own size with the strip outside the crop
counted as background.  The reference has that step in post_processing/crf_refine.py:84-97 (run_crf_original_resolution) and
post_processing/post_processing.py:32-46:

    soft = imresize(soft, (int(0.9 H), int(0.9 W)));  soft = soft / (amax(soft) + 1e-8);  zeros((H, W))[dh:dh+h, dw:dw+w] = soft

  restore_box(H, W, crop)                       the patch's box (y0, x0, h, w) inside an H x W frame
  build_restore_tables / check_restore_tables   the host tables of udet_restore_masks_ragged and their validation (no GPU needed)
  restore_masks(masks, native_hw, ...)          one call of the ragged kernel -> RestoredMasks: buffers of one batch in one
                                                ragged.PackedLayout (the packed layout)

scipy.misc.imresize is restated as bytescale + Pillow's 8-bit bilinear resampler."""
import ctypes

import numpy as np
import torch

from . import ragged
from ._ffi import c_i, c_p, c_sz, check, lib, sig
from .pil_tables import CoefBlocks, check_pass
from .ragged import PackedLayout, PackedSamples, as_layout, check_packed_tables, require_tensor, workspace

sig("udet_restore_workspace_bytes", c_sz, c_i)
sig("udet_restore_masks_ragged", c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, ctypes.c_double, c_p, c_sz, c_p)

TAB = 12  # int32 per sample: y0 x0 h w H W | hk hb hks | vk vb vks   (include/udet.h)


def restore_box(H, W, crop):
    """(y0, x0, h, w) of the restored patch in an H x W frame: h = int(H * crop), w = int(W * crop) (Python float product,
    truncated, crf_refine.py:91-92), y0 = (H - h) // 2, x0 = (W - w) // 2; crop >= 1: the whole frame.  h, w >= 1."""
    H, W, crop = int(H), int(W), float(crop)
    if H < 1 or W < 1 or not crop > 0:
        raise ValueError("restore_box: frame {} x {} and crop {} must be positive".format(H, W, crop))
    if crop >= 1:
        return 0, 0, H, W
    h, w = int(H * crop), int(W * crop)
    if h < 1 or w < 1:
        raise ValueError("restore_box: the crop {} of a {} x {} frame is empty".format(crop, H, W))
    return (H - h) // 2, (W - w) // 2, h, w


def build_restore_tables(native_hw, mh, mw, crop=0.9, offsets=None):
    """Host tables of udet_restore_masks_ragged for masks of mh x mw restored into frames native_hw [n,2]: (offsets int64 [n],
    tab int32 [n,12], coef int32 [m]).  offsets default to the packed layout (sample i right after sample i-1).  One coefficient
    table (kk [out][ks] then bounds [out][2]) per distinct (in, out) length, concatenated in coef; a pass whose output length
    equals its input length gets index -1 (skipped)."""
    hw = np.asarray(native_hw, dtype=np.int64).reshape(-1, 2)
    n = len(hw)
    if n < 1:
        raise ValueError("restore needs at least one sample")
    if offsets is None:
        off = PackedLayout.packed(hw).offsets
    else:
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        if len(off) != n:
            raise ValueError("one offset per sample")
    tab = np.zeros((n, TAB), np.int32)
    blocks = CoefBlocks()
    for i, (H, W) in enumerate(hw):
        y0, x0, h, w = restore_box(H, W, crop)
        tab[i] = (y0, x0, h, w, H, W) + blocks.block(mw, w) + blocks.block(mh, h)
    return off, tab, blocks.coef()


def check_restore_tables(offsets, tab, coef, numel, mh, mw):
    """Host validation of the device tables of udet_restore_masks_ragged (its C entry point does not read device memory): raises
    ValueError on tables ragged.check_packed_tables refuses for an output buffer of `numel` bytes, a box outside its own frame, a
    coefficient window outside coef, or a tap outside the mask.  Returns the three arrays in the dtypes the kernel reads."""
    tab = np.ascontiguousarray(np.asarray(tab, dtype=np.int32).reshape(-1, TAB))
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.int32).reshape(-1))
    if mh < 1 or mw < 1:
        raise ValueError("restore needs a mask of at least 1x1")
    t = tab.astype(np.int64)
    y0, x0, h, w, H, W = (t[:, k] for k in range(6))
    off, _ = check_packed_tables(offsets, t[:, 4:6], numel, buffer="output buffer")
    n = len(off)
    if (y0 < 0).any() or (x0 < 0).any() or (h < 1).any() or (w < 1).any() or (y0 + h > H).any() or (x0 + w > W).any():
        raise ValueError("box outside its own frame")
    for i in range(n):
        for name, block, n_in, n_out in (("horizontal", t[i, 6:9], mw, w[i]), ("vertical", t[i, 9:12], mh, h[i])):
            check_pass(coef, block, n_in, n_out, "sample {}".format(i), name)
    return off, tab, coef


class RestoredMasks(PackedSamples):
    """Result of restore_masks: data (packed uint8, device), binary (same layout, 0 / 1, or None), amax (device int32 [n]); their
    `layout` is given as host offsets [n] / hw [n,2], or as the PackedLayout itself (hw=None)."""

    def __init__(self, data, binary, offsets, hw, amax):
        PackedSamples.__init__(self, as_layout(offsets, hw, data.numel()), data.device)
        self.data, self.binary, self.amax = data, binary, amax

    def sample(self, i):
        """[H_i, W_i] uint8 view of sample i."""
        return self._view(self.data, i)

    def binary_sample(self, i):
        if self.binary is None:
            raise ValueError("restored without a threshold: no binary mask")
        return self._view(self.binary, i)

    def soft(self, i):
        """float64 [H_i, W_i] = byte / (amax + 1e-8): the mask run_crf_original_resolution hands to its CRF (crf_refine.py:94)."""
        return self.sample(i).double() / (self.amax[i].double() + 1e-8)


# Everything the restore tables are built from -> [the layout of a call that gave none, off, tab, coef, {device: (tab, coef) there}]: a
# batch with the sizes of an earlier one (every DAVIS batch) has its tables built, validated and uploaded once.
_restore_tables = {}


def restore_masks(masks, native_hw, crop=0.9, threshold=None, offsets=None, out=None, binary_out=None) -> RestoredMasks:
    """n soft masks [n,mh,mw] or [n,mh,mw,1] (device float32, or an array) -> each restored to its own native_hw[i] = (H_i, W_i):
    bytescale over the whole mask, Pillow's 8-bit bilinear resize to restore_box(H_i, W_i, crop), pasted into zeros; amax[i] = the
    patch's largest byte; threshold (float, optional): also the binary mask byte / (amax + 1e-8) > threshold (float64).  One call
    of udet_restore_masks_ragged: at most three launches for the whole batch.  offsets / out / binary_out: a caller-owned packed
    uint8 buffer and the byte offset of every sample in it (default: a fresh buffer, samples back to back).  native_hw may be the
    PackedLayout of the output (the annotations' own: its sizes, offsets and device tables are used as they are).  The tables are
    validated on the host before anything is launched (ValueError)."""
    m = masks if isinstance(masks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32))
    if m.dim() == 4 and m.shape[-1] == 1:
        m = m[..., 0]
    if m.dim() != 3:
        raise ValueError("masks must be [n,mh,mw] or [n,mh,mw,1]")
    n, mh, mw = (int(v) for v in m.shape)
    given = native_hw if isinstance(native_hw, PackedLayout) else None
    hw = np.asarray(native_hw, dtype=np.int64).reshape(-1, 2)
    if len(hw) != n or (given is not None and offsets is not None):
        raise ValueError("one native size per mask (a PackedLayout brings its own offsets)")
    if given is not None:
        offsets = given.offsets
    total = int(out.numel()) if out is not None else (int((hw[:, 0] * hw[:, 1]).sum()) if given is None else given.numel)
    if threshold is not None and not (0.0 <= float(threshold) < float("inf")):
        raise ValueError("threshold must be finite and >= 0")
    key = (hw.tobytes(), None if offsets is None else np.asarray(offsets, dtype=np.int64).tobytes(), total, mh, mw, float(crop))
    if key not in _restore_tables:  # before the device is touched
        off, tab, coef = check_restore_tables(*build_restore_tables(hw, mh, mw, crop, offsets), total, mh, mw)
        if len(_restore_tables) >= 16:
            _restore_tables.clear()
        _restore_tables[key] = [None, off, tab, coef, {}]
    entry = _restore_tables[key]
    if given is None and entry[0] is None:
        entry[0] = PackedLayout(entry[1], hw, total, buffer="output buffer")
    layout = entry[0] if given is None else as_layout(given, None, total, buffer="output buffer")
    tab, coef, on_device = entry[2:]
    m = m.to("cuda", torch.float32).contiguous()
    dev = m.device
    for buf, name in ((out, "out"), (binary_out, "binary_out")):
        if buf is not None:
            require_tensor(buf, name + " (the output buffer)", torch.uint8, 1, total)
    data = torch.empty(total, dtype=torch.uint8, device=dev) if out is None else out
    binary = None
    if threshold is not None:
        binary = torch.empty(total, dtype=torch.uint8, device=dev) if binary_out is None else binary_out
    if dev not in on_device:
        on_device[dev] = ragged.upload_tables([tab, coef], dev)
        torch.cuda.current_stream(dev).synchronize()  # once per table set: a later call may run on another stream
    (d_tab, d_coef), (d_off, _) = on_device[dev], layout.device_tables(dev)
    amax = torch.empty(n, dtype=torch.int32, device=dev)  # zeroed by the call
    ws = workspace(lib.udet_restore_workspace_bytes(n), 4, dev)
    check(lib.udet_restore_masks_ragged(m.data_ptr(), n, mh, mw, d_off.data_ptr(), d_tab.data_ptr(), d_coef.data_ptr(),
                                        layout.max_h, layout.max_w, data.data_ptr(), amax.data_ptr(),
                                        None if binary is None else binary.data_ptr(), 0.0 if threshold is None else float(threshold),
                                        ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return RestoredMasks(data, binary, layout, None, amax)
