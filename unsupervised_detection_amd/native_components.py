"""Native-resolution stage, step 2: connected components of the restored masks and the choice of one candidate per sample
(csrc/components.hip) -- the "best detection candidate from the set of predicted connected masks" the reference only
mentions in a comment (post_processing.py:32-35).

  select_components(binary, offsets, hw, gt, mode, ...)   one call of udet_select_components_ragged -> ComponentSelection: buffers of
                                                one batch in one ragged.PackedLayout (the packed layout)
  check_component_tables                        the host validation of its device tables (no GPU needed)
  packed_labels(selection_or_labels, offsets, hw)   the labels and the layout the later steps (native_detections, native_tracks) take:
                                                from a ComponentSelection, or a raw tensor with its tables"""
import numpy as np
import torch

from ._ffi import c_i, c_p, c_sz, check, lib, sig
from .native_restore import RestoredMasks
from .ragged import PackedLayout, PackedSamples, as_layout, check_packed_tables, require_tensor, workspace

sig("udet_components_workspace_bytes", c_sz, c_sz, c_i)
sig("udet_select_components_ragged", c_i, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_i, c_i, c_p, c_p, c_p, c_p, c_sz, c_p)

COMPONENT_MODES = {"label": 0, "largest": 1, "best_gt": 2}  # UDET_COMPONENTS_LABEL / _LARGEST / _BEST_GT (include/udet.h)
COMPONENT_TILE = (32, 64)  # UDET_COMPONENTS_TILE_H / _W: the tile of the LDS union-find


def check_component_tables(offsets, hw, numel):
    """Host validation of the device tables of udet_select_components_ragged: ragged.check_packed_tables for a packed buffer of
    `numel` elements.  Returns (offsets int64 [n], hw int32 [n,2]) as the kernels read them."""
    return check_packed_tables(offsets, hw, numel)


class ComponentSelection(PackedSamples):
    """Result of select_components: selected (packed uint8 0 / 1, device; None in mode "label"), labels (packed int32, root + 1 /
    0, or None), info (device int64 [n,4] = components, chosen root or -1, its area, its inter); their `layout` is given as host
    offsets [n] / hw [n,2], or as the PackedLayout itself (hw=None).  binary_sample / stack have the contract of RestoredMasks: the
    scoring and export loops take either."""

    def __init__(self, selected, labels, info, offsets, hw):
        if isinstance(offsets, PackedLayout) or selected is not None or labels is not None:
            numel = offsets.numel if isinstance(offsets, PackedLayout) else (labels if selected is None else selected).numel()
        else:  # no packed buffer to measure: the tables' own extent
            numel = int((np.asarray(offsets, np.int64).reshape(-1) + np.asarray(hw, np.int64).reshape(-1, 2).prod(1)).max())
        PackedSamples.__init__(self, as_layout(offsets, hw, numel), info.device)
        self.selected, self.labels, self.info = selected, labels, info

    def binary_sample(self, i):
        if self.selected is None:
            raise ValueError("labelled without a selection: no selected mask")
        return self._view(self.selected, i)

    def labels_sample(self, i):
        if self.labels is None:
            raise ValueError("selected without want_labels: no labels")
        return self._view(self.labels, i)


def packed_labels(selection_or_labels, offsets=None, hw=None):
    """(labels, offsets, hw) of what the steps after the labelling take: a ComponentSelection that has labels (its own layout comes back
    as offsets, hw=None), or a packed label tensor with host offsets [n] / hw [n,2] or a PackedLayout as offsets (ValueError otherwise)."""
    if isinstance(selection_or_labels, ComponentSelection):
        if selection_or_labels.labels is None:
            raise ValueError("selected without want_labels: no labels")
        if offsets is not None or hw is not None:
            raise ValueError("a ComponentSelection brings its own layout")
        return selection_or_labels.labels, selection_or_labels.layout, None
    if offsets is None or (hw is None and not isinstance(offsets, PackedLayout)):
        raise ValueError("a packed buffer needs its offsets and sizes")
    return selection_or_labels, offsets, hw


def select_components(binary, offsets=None, hw=None, gt=None, mode="largest", connectivity=8, want_labels=False) -> ComponentSelection:
    """Connected components of n packed binary masks and one of them chosen per sample, in one call of
    udet_select_components_ragged (five launches whatever n is).  binary: a RestoredMasks (its binary masks and layout), or a 1-D
    uint8 device tensor with host offsets [n] / hw [n,2] (or a PackedLayout as offsets, hw=None: taken as it is); gt: a
    native_results.GtBatch (any PackedSamples with the 0 / 1 bytes as `data`) or a 1-D uint8 device tensor packed like binary, or None.
    connectivity 4 or 8.  mode "label": components only; "largest": the largest component, ties to the smaller root (the
    smallest row-major index of the component); "best_gt": the largest IoU with gt, ties to the larger area, then the smaller root.
    want_labels: also the int32 labels (root + 1, background 0; the roots in ascending order number as scipy.ndimage.label does).
    Arguments and tables are validated on the host before the device is touched (ValueError)."""
    if isinstance(binary, RestoredMasks):
        if binary.binary is None:
            raise ValueError("restored without a threshold: no binary mask")
        binary, offsets, hw = binary.binary, binary.layout, None
    if offsets is None or (hw is None and not isinstance(offsets, PackedLayout)):
        raise ValueError("a packed buffer needs its offsets and sizes")
    if mode not in COMPONENT_MODES:
        raise ValueError("mode must be one of {}".format(sorted(COMPONENT_MODES)))
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    total = int(require_tensor(binary, "binary (packed samples)", torch.uint8, 1, cuda=False).numel())
    layout = as_layout(offsets, hw, total)  # raw tables: validated before the device is touched
    if isinstance(gt, PackedSamples):
        if not gt.layout.same_as(layout):
            raise ValueError("the annotations must be packed like the masks (same offsets and sizes)")
        gt = gt.data
    if mode == "best_gt" and gt is None:
        raise ValueError('mode "best_gt" needs the annotations')
    dev, n = binary.device, layout.n
    if gt is not None:
        require_tensor(gt, "gt (packed like binary)", torch.uint8, 1, total, dev)
    require_tensor(binary, "binary (packed samples)", torch.uint8, 1)
    d_off, d_hw = layout.device_tables(dev)
    selected = torch.empty(total, dtype=torch.uint8, device=dev) if mode != "label" else None
    labels = torch.empty(total, dtype=torch.int32, device=dev) if want_labels else None
    info = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ws = workspace(lib.udet_components_workspace_bytes(total, n), 8, dev)
    check(lib.udet_select_components_ragged(binary.data_ptr(), None if gt is None else gt.data_ptr(), n, d_off.data_ptr(), d_hw.data_ptr(),
                                            layout.max_h, layout.max_w, total, int(connectivity), COMPONENT_MODES[mode],
                                            None if labels is None else labels.data_ptr(), None if selected is None else selected.data_ptr(),
                                            info.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return ComponentSelection(selected, labels, info, layout, None)
