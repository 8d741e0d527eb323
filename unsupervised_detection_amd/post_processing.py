"""Post-processing stage of the reference on the GPU ("next" row N4 of SURVEY.md section 8f), same function names and argument
meaning as post_processing/generate_soft_score_from_buffer.py and post_processing/crf_refine.py:

  sanity_check(s) / rectify_pred_mask(pred_mask, crop, H, W)      generate_soft_score_from_buffer.py:116-125, :98-114
  soft_score(...)   the per-frame body of buffer_to_soft_score   :38-93  (device tensors in, device tensor out: no .mat round trip)
  propagate(...)    flow-guided moving average of the masks       :127-231 (pyflow.so -> the path's own PWC-Net flow; cv2.remap -> udet_post_remap)
  refine(...) / select_candidate(...)                             crf_refine.py:110-138, :40-50
  buffer_to_soft_score(buffer_path, out_path, ...) / run_crf(...)  the file-level drivers over the .mat buffers the ensemble run writes
  dense_crf_ragged(...) / unary_from_restored(...) / run_crf_original_resolution(...)   crf_refine.py:65-108: the CRF on every frame at
                    its own size, a ragged batch per call (csrc/crf.hip) in the packed layout of ragged.py:
                    both take host offsets / hw, or the batch's PackedLayout and then neither validate nor upload
  propagate_sequences(...) / PWCFlow.batch(...) / select_unary_batch(...)   the sequence stage batched (csrc/sequence.hip):
                    propagate(flow_batch=), buffer_to_soft_score(flow_batch=) and run_crf(batch=) reach them; the defaults (None) keep the
                    per-frame paths
  soft_score_batch(...) / soft_score_geometry(...)   soft_score for a batch of frames in four launches (csrc/soft_score.hip):
                    buffer_to_soft_score(score_batch=) reaches it; the default (None) keeps the per-frame path

The kernels of the stage -- border statistics, bytescale, Pillow's 8-bit resampler, canvas placement, min-max / max
normalisations, remap, blending, the separable Gaussian and the dense-CRF mean field -- run in libudet.so (csrc/postproc.hip); torch
holds the device memory and does a few elementwise glue steps (adding two score maps, clamp / log of the unary).  What the reference
delegates to third-party code that is not in its tree (scipy.misc.imresize, cv2.remap, pyflow, pydensecrf) is restated from the
published algorithms -- see oracle/oracle_post.py for the restatement the kernels are tested against and for what could and could
not be pinned to the original libraries."""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from ._ffi import c_f, c_i, c_p, c_sz, check, lib, sig
from .pil_tables import CoefBlocks, check_pass, pil_coeffs_host as _pil_coeffs_host
from .ragged import INT32_MAX, PackedLayout, as_layout, check_ranges, require_tensor, upload_tables, workspace

c_d = ctypes.c_double

for _n, _a in (("udet_post_border_mean", [c_p, c_i, c_i, c_i, c_p, c_p]),
               ("udet_post_bytescale", [c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
               ("udet_post_resample_u8", [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_p]),
               ("udet_post_place", [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p]),
               ("udet_post_minmax_norm", [c_p, c_i, c_p, c_p]),
               ("udet_post_remap", [c_p, c_p, c_p, c_i, c_i, c_p]),
               ("udet_post_blend", [c_p, c_f, c_p, c_f, c_i, c_i, c_p]),
               ("udet_post_gauss1d", [c_p, c_p, c_i, c_i, c_p, c_i, c_i, c_p]),
               ("udet_post_dense_crf", [c_p, c_p, c_i, c_i, c_f, c_f, c_f, c_i, c_i, c_p, c_p, c_sz, c_p]),
               # the dense CRF of a ragged batch at native resolution (csrc/crf.hip)
               ("udet_dense_crf_ragged", [c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_f, c_f, c_f, c_i, c_i, c_p, c_p, c_p, c_sz, c_p]),
               ("udet_dense_crf_rows_per_thread", [c_i, c_i, c_i]),
               ("udet_crf_unary_lookup", [c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_sz, c_p, c_p]),
               # the sequence stage, batched (csrc/sequence.hip)
               ("udet_post_propagate_sequences", [c_p, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_p, c_p, c_p, c_sz, c_p]),
               ("udet_post_select_unary", [c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
               # the soft scores of a batch of frames (csrc/soft_score.hip)
               ("udet_post_soft_score_batch", [c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_d, c_p, c_p, c_sz, c_p])):
    sig(_n, c_i, *_a)
sig("udet_post_soft_score_workspace_bytes", c_sz, c_i, c_i, c_i, c_i, c_i)
sig("udet_post_crf_workspace_bytes", c_sz, c_i, c_i)
sig("udet_dense_crf_workspace_bytes", c_sz, c_sz, c_i)
sig("udet_post_propagate_workspace_bytes", c_sz, c_i, c_i)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x, dtype):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to("cuda", dtype).contiguous()


def _as_mask(m):
    """A soft mask as the stage takes it: its singleton dimensions dropped, device float32."""
    return _dev(m.squeeze() if isinstance(m, torch.Tensor) else np.squeeze(m), torch.float32)


# ---------------------------------------------------------------------------------------------- Pillow coefficients ----
_coeff_cache = {}


def _pil_coeffs(in_size: int, out_size: int):
    """_pil_coeffs_host as device int32 tables kk [out][ksize] and bounds [out][2] (cached per (in, out))."""
    key = (in_size, out_size)
    if key not in _coeff_cache:
        kk, bounds, ksize = _pil_coeffs_host(in_size, out_size)
        _coeff_cache[key] = (torch.from_numpy(kk).cuda(), torch.from_numpy(bounds).cuda(), ksize)
    return _coeff_cache[key]


def _imresize_window(src64: torch.Tensor, y0, x0, h, w, out_h, out_w) -> torch.Tensor:
    """scipy.misc.imresize(src[y0:y0+h, x0:x0+w], (out_h, out_w)) -> uint8 device tensor [out_h, out_w]."""
    H, W = src64.shape
    u8 = torch.empty((h, w), dtype=torch.uint8, device=src64.device)
    check(lib.udet_post_bytescale(src64.data_ptr(), W, y0, x0, h, w, u8.data_ptr(), _stream()))
    cur, ch, cw = u8, h, w
    if out_w != cw:
        kk, bounds, ks = _pil_coeffs(cw, out_w)
        nxt = torch.empty((ch, out_w), dtype=torch.uint8, device=src64.device)
        check(lib.udet_post_resample_u8(cur.data_ptr(), ch, cw, nxt.data_ptr(), ch, out_w, kk.data_ptr(), bounds.data_ptr(), ks, 1, _stream()))
        cur, cw = nxt, out_w
    if out_h != ch:
        kk, bounds, ks = _pil_coeffs(ch, out_h)
        nxt = torch.empty((out_h, cw), dtype=torch.uint8, device=src64.device)
        check(lib.udet_post_resample_u8(cur.data_ptr(), ch, cw, nxt.data_ptr(), out_h, cw, kk.data_ptr(), bounds.data_ptr(), ks, 0, _stream()))
        cur = nxt
    return cur


# ------------------------------------------------------------------------------------------------------ soft score ----
def sanity_check(s):
    """mean over the four two-pixel border strips (generate_soft_score_from_buffer.py:116-125); s: [H,W] or [N,H,W] -> float / array."""
    t = _dev(s, torch.float32)
    single = t.dim() == 2
    t = t.view(-1, t.shape[-2], t.shape[-1])
    out = torch.empty(t.shape[0], dtype=torch.float64, device=t.device)
    check(lib.udet_post_border_mean(t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], out.data_ptr(), _stream()))
    v = out.cpu().numpy()
    return float(v[0]) if single else v


def rectify_pred_mask(pred_mask, crop, H, W):
    """Bring a prediction made on another central crop back to the base crop (:98-114) -> device float64 [H,W]."""
    p = _dev(pred_mask, torch.float64)
    canvas = torch.empty((H, W), dtype=torch.float64, device=p.device)
    if crop > 1:
        crop = 1.0 / crop
        hh, ww = int(H * crop), int(W * crop)
        h, w = int((H - hh) / 2), int((W - ww) / 2)
        patch = _imresize_window(p, h, w, hh, ww, H, W)
        check(lib.udet_post_place(patch.data_ptr(), H, W, 0, 0, H, W, canvas.data_ptr(), _stream()))
    else:
        hh, ww = int(H * crop), int(W * crop)
        patch = _imresize_window(p, 0, 0, p.shape[0], p.shape[1], hh, ww)
        h, w = max(int((H - hh) / 2), 0), max(int((W - ww) / 2), 0)
        check(lib.udet_post_place(patch.data_ptr(), hh, ww, h, w, H, W, canvas.data_ptr(), _stream()))
    return canvas


def soft_score(preds_b, preds_f, crops=(85, 90, 95, 100), base_crop=90.0, base_hw=(192, 384), san_t=0.6):
    """The per-frame body of buffer_to_soft_score (:38-93).  preds_b / preds_f: [shift-1][crop index] soft masks [H,W] (device
    tensors or arrays) of the backward (-shift) / forward (+shift) ensemble runs -> pred_mask, device float64 [H,W]."""
    H, W = base_hw
    ns, nc = len(preds_b), len(crops)
    allm = torch.stack([_as_mask(m) for grp in (preds_b, preds_f) for row in grp for m in row], 0)
    sani = sanity_check(allm).reshape(2, ns, nc)  # one launch for every mask of the frame
    score = None
    for si in range(ns):
        for ci, crop in enumerate(crops):
            s_b, s_f = allm[si * nc + ci], allm[(ns + si) * nc + ci]
            bad_b, bad_f = sani[0, si, ci] >= san_t, sani[1, si, ci] >= san_t
            if bad_b and bad_f:
                s_b, s_f = torch.zeros_like(s_b), torch.zeros_like(s_f)
            elif bad_b:
                s_b = s_f
            elif bad_f:
                s_f = s_b
            if si == 0 and crop == base_crop:
                term = s_b.double() + s_f.double()
            else:
                ratio = crop / base_crop
                term = rectify_pred_mask(s_b, ratio, H, W) + rectify_pred_mask(s_f, ratio, H, W)
            score = term if score is None else score + term
    out = torch.empty_like(score)
    check(lib.udet_post_minmax_norm(score.data_ptr(), score.numel(), out.data_ptr(), _stream()))
    return out


# ---------------------------------------------------------------------------------------------- soft score, batched ----
SOFT_SCORE_GEOM = 16  # UDET_SOFT_SCORE_GEOM (include/udet.h): mode | sy0 sx0 sh sw | hh ww y0 x0 | hk hb hks | vk vb vks | 0
_soft_tables = {}


def soft_score_geometry(ns, crops, base_crop, base_hw):
    """The tables of udet_post_soft_score_batch (pure host): geom int32 [ns * len(crops), SOFT_SCORE_GEOM], one row per (shift index, crop
    index) with rectify_pred_mask's integer rules (int(H * crop), int((H - hh) / 2), max(..., 0), the crop > 1 branch), and coef int32, the
    concatenated coefficient blocks of pil_tables.CoefBlocks (kk then bounds, one pair per distinct (in, out) size) the rows' offsets point into.  Row layout:
    mode (0: shift 1 at the base crop, the raw masks; 1: rectify), the source window (sy0, sx0, sh, sw) inside the mask, the patch (hh, ww)
    and where it lands (y0, x0), then (kk offset, bounds offset, ksize) of the horizontal and of the vertical pass, a negative offset for a
    pass whose output is as long as its input."""
    H, W = (int(v) for v in base_hw)
    ns, nc = int(ns), len(crops)
    if ns < 1 or nc < 1 or H < 1 or W < 1:
        raise ValueError("soft_score_geometry: at least one shift, one crop and a frame of 1 x 1")
    geom = np.zeros((ns * nc, SOFT_SCORE_GEOM), np.int32)
    blocks = CoefBlocks()
    for si in range(ns):
        for ci, crop in enumerate(crops):
            r = si * nc + ci
            if si == 0 and crop == base_crop:
                geom[r, :9] = (0, 0, 0, H, W, H, W, 0, 0)
                geom[r, 9:15] = (-1, -1, 0, -1, -1, 0)
                continue
            ratio = crop / base_crop
            if ratio > 1:  # a central window of the mask, enlarged to the whole canvas
                c = 1.0 / ratio
                hh, ww = int(H * c), int(W * c)
                win, patch = (int((H - hh) / 2), int((W - ww) / 2), hh, ww), (H, W, 0, 0)
            else:          # the whole mask, shrunk and placed on the canvas
                hh, ww = int(H * ratio), int(W * ratio)
                win, patch = (0, 0, H, W), (hh, ww, max(int((H - hh) / 2), 0), max(int((W - ww) / 2), 0))
            if hh < 1 or ww < 1:
                raise ValueError("soft-score geometry row {} (shift {}, crop {}): a frame of {} x {} leaves no pixel".format(r, si + 1, crop, H, W))
            geom[r, :9] = (1,) + win + patch
            geom[r, 9:15] = blocks.block(win[3], patch[1]) + blocks.block(win[2], patch[0])
    return geom, blocks.coef()


def check_soft_score_tables(geom, coef, base_hw):
    """Host validation of the tables of udet_post_soft_score_batch, before the device is touched (the kernels take every index from them):
    ValueError, naming the row, unless every rectify row's source window and patch lie inside the H x W frame, its coefficient blocks
    inside coef, and every tap inside the window (first taps and ends non-decreasing, as Pillow's are).  Returns (geom, coef) as
    contiguous int32 arrays."""
    H, W = (int(v) for v in base_hw)
    g = np.ascontiguousarray(np.asarray(geom, dtype=np.int64))
    co = np.ascontiguousarray(np.asarray(coef, dtype=np.int64).reshape(-1))
    if g.ndim != 2 or g.shape[1] != SOFT_SCORE_GEOM or len(g) < 1 or len(co) < 1:
        raise ValueError("soft-score tables: geom must be [rows, {}] with at least one row, coef not empty".format(SOFT_SCORE_GEOM))
    if (np.abs(g) > INT32_MAX).any() or (np.abs(co) > INT32_MAX).any():
        raise ValueError("soft-score tables: values must fit int32")
    for r, row in enumerate(g.tolist()):
        mode, sy0, sx0, sh, sw, hh, ww, y0, x0 = row[:9]
        if mode not in (0, 1):
            raise ValueError("soft-score geometry row {}: mode must be 0 (identity) or 1 (rectify)".format(r))
        if mode == 0:
            continue
        if min(sy0, sx0) < 0 or min(sh, sw) < 1 or sy0 + sh > H or sx0 + sw > W:
            raise ValueError("soft-score geometry row {}: the source window {}x{} at ({}, {}) leaves the {}x{} frame".format(r, sh, sw, sy0, sx0, H, W))
        if min(y0, x0) < 0 or min(hh, ww) < 1 or y0 + hh > H or x0 + ww > W:
            raise ValueError("soft-score geometry row {}: the patch {}x{} at ({}, {}) leaves the {}x{} canvas".format(r, hh, ww, y0, x0, H, W))
        for name, block, n_in, n_out in (("horizontal", row[9:12], sw, ww), ("vertical", row[12:15], sh, hh)):
            check_pass(co, block, n_in, n_out, "soft-score geometry row {}".format(r), name)
    return g.astype(np.int32), co.astype(np.int32)


def _soft_score_tables(ns, crops, base_crop, H, W, device):
    """Device copies of soft_score_geometry's validated tables, cached per (ns, crops, base_crop, H, W) and device."""
    key = (ns, tuple(crops), float(base_crop), H, W, device)
    if key not in _soft_tables:
        geom, coef = check_soft_score_tables(*soft_score_geometry(ns, crops, base_crop, (H, W)), base_hw=(H, W))
        _soft_tables[key] = tuple(upload_tables([geom.reshape(-1), coef], device))
        torch.cuda.current_stream(device).synchronize()  # once per key: a later call may run on another stream
    return _soft_tables[key]


def soft_score_batch(preds, crops=(85, 90, 95, 100), base_crop=90.0, san_t=0.6):
    """soft_score for n frames in one call of udet_post_soft_score_batch: four launches whatever n is, no host synchronisation and no copy
    to the host.  preds: [n, 2, ns, nc, H, W] (device tensor or array), preds[i, 0] / preds[i, 1] = frame i's preds_b / preds_f with nc =
    len(crops); the frame is the masks' own H x W.  Returns device float64 [n, H, W], row i bit-identical to soft_score(preds[i, 0],
    preds[i, 1], crops, base_crop, (H, W), san_t)."""
    t = _dev(preds, torch.float32)
    if t.dim() != 6 or t.shape[1] != 2 or t.shape[3] != len(crops) or t.shape[0] < 1:
        raise ValueError("preds must be [n, 2, ns, {}, H, W] (one mask per direction, shift and crop), n at least 1".format(len(crops)))
    n, _, ns, nc, H, W = (int(v) for v in t.shape)
    d_geom, d_coef = _soft_score_tables(ns, crops, base_crop, H, W, t.device)
    out = torch.empty((n, H, W), dtype=torch.float64, device=t.device)
    ws = workspace(lib.udet_post_soft_score_workspace_bytes(n, ns, nc, H, W), 16, t.device)
    check(lib.udet_post_soft_score_batch(t.data_ptr(), n, ns, nc, H, W, d_geom.data_ptr(), d_coef.data_ptr(), float(san_t), out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream(t.device).cuda_stream))
    return out


# ------------------------------------------------------------------------------------------------------ propagation ----
def remap(src, flow_uv):
    """cv2.remap(src, flow_uv + pixel grid, None, cv2.INTER_LINEAR) (:171-176): src [H,W] float32, flow_uv [H,W,2] = (u, v)."""
    s, f = _dev(src, torch.float32), _dev(flow_uv, torch.float32)
    H, W = s.shape
    out = torch.empty_like(s)
    check(lib.udet_post_remap(s.data_ptr(), f.data_ptr(), out.data_ptr(), H, W, _stream()))
    return out


def propagate_step(running_avg, s_prev, flow_uv, w_r=0.85):
    """One step of propagate (:166-185): pull the previous mask and the running average along flow_uv to the current frame and
    blend them; every intermediate is max-normalised like the reference.  Returns the new running average (device float32)."""
    s2 = remap(s_prev, flow_uv)
    ra_w = remap(running_avg, flow_uv)
    ra = torch.empty_like(ra_w)
    n = ra.numel()
    check(lib.udet_post_blend(ra_w.data_ptr(), 1.0, ra.data_ptr(), 0.0, n, 0, _stream()))                 # ra = ra_w / (max + 1e-8)
    check(lib.udet_post_blend(s2.data_ptr(), float(np.float32(1 - w_r)), ra.data_ptr(), float(np.float32(w_r)), n, 1, _stream()))
    return ra


class PWCFlow(object):
    """Replacement of pyflow.coarse2fine_flow in propagate(): the path's own PWC-Net.  flow(I_from, I_to) returns
    (u, v) [H,W,2] such that I_from(x, y) ~ I_to(x + u, y + v) -- the convention of the call at :158-160."""

    def __init__(self, model=None):
        from .functional import ModelPWCNet
        self.model = model or ModelPWCNet()

    def __call__(self, img_from_u8, img_to_u8):
        a = _dev(img_from_u8, torch.float32) / 255.0 - 0.5
        b = _dev(img_to_u8, torch.float32) / 255.0 - 0.5
        # the trained network's channel 0 is u (the x displacement of the ground-truth flows it was fitted to), channel 1 is v:
        # the order pyflow returns and cv2.remap's map expects (:162-165)
        return self.model.predict_from_img_pairs(a.unsqueeze(0).contiguous(), b.unsqueeze(0).contiguous())[0].contiguous()

    def batch(self, imgs_from, imgs_to, batch=8):
        """The flows of many pairs, `batch` pairs per network call: imgs_from / imgs_to are equally long lists of [H,W,3] uint8 frames ->
        device float32 [n,H,W,2], row i = self(imgs_from[i], imgs_to[i])'s field.  Every call has `batch` pairs (the last chunk is
        padded by repeating its last pair, flow_chunks), so one engine shape is built whatever n is."""
        if len(imgs_from) != len(imgs_to) or not len(imgs_from):
            raise ValueError("as many frames to start from as to go to, and at least one pair")
        out = None
        for idx, keep in flow_chunks(len(imgs_from), batch):
            a = torch.stack([_dev(imgs_from[i], torch.float32) for i in idx], 0) / 255.0 - 0.5
            b = torch.stack([_dev(imgs_to[i], torch.float32) for i in idx], 0) / 255.0 - 0.5
            f = self.model.predict_from_img_pairs(a.contiguous(), b.contiguous())
            if out is None:
                out = torch.empty((len(imgs_from),) + tuple(f.shape[1:]), dtype=torch.float32, device=f.device)
            out[idx[0]:idx[0] + keep] = f[:keep]
        return out


def flow_chunks(n, batch):
    """The chunking of PWCFlow.batch: n pairs in calls of exactly `batch` -> [(indices [batch], keep), ...]; the indices of a chunk are
    consecutive, its first `keep` results are used, and the last chunk is padded with its last pair's index."""
    n, batch = int(n), int(batch)
    if n < 1 or batch < 1:
        raise ValueError("flow_chunks: n and batch must be at least 1")
    out = []
    for lo in range(0, n, batch):
        keep = min(batch, n - lo)
        out.append((list(range(lo, lo + keep)) + [lo + keep - 1] * (batch - keep), keep))
    return out


def check_sequence_tables(seq_first, seq_len, total):
    """Host validation of the device tables of udet_post_propagate_sequences, before the device is touched: raises ValueError unless
    every sequence has at least one frame, lies inside the array of `total` frames and shares no frame with another one (any order, gaps
    allowed); at most 65535 sequences.  Returns (seq_first, seq_len) as int32 arrays [n_seq], as the kernels read them."""
    first, length = np.asarray(seq_first, dtype=np.int64).reshape(-1), np.asarray(seq_len, dtype=np.int64).reshape(-1)
    if len(first) != len(length) or not 1 <= len(first) <= 65535:
        raise ValueError("one first frame and one length per sequence, 1..65535 sequences")
    if int(total) < 1 or int(total) > 0x7fffffff:
        raise ValueError("total frames must be in 1..2^31-1")
    if (length < 1).any():
        raise ValueError("a sequence has a length below 1")
    check_ranges(first, length, int(total), "sequence", "array of {} frames".format(int(total)))
    return first.astype(np.int32), length.astype(np.int32)


def propagate_sequences(masks, flow_prev, flow_next, seq_lens, w_r=0.85):
    """propagate() for many sequences in one call of udet_post_propagate_sequences (two launches whatever the batch), given the flows.
    masks: device float32 [total,H,W], the sequences one after the other (seq_lens: their lengths, host integers summing to total);
    flow_prev / flow_next: device float32 [total,H,W,2], (u, v) from frame k to k - 1 / k + 1 (the entry of a sequence's first / last frame
    is not read).  Returns (avg_f, avg_b), device float32 [total,H,W]: bit-identical to propagate()'s lists with the same flows."""
    for t, nd, name in ((masks, 3, "masks"), (flow_prev, 4, "flow_prev"), (flow_next, 4, "flow_next")):
        require_tensor(t, name, torch.float32, nd)
    total, H, W = (int(v) for v in masks.shape)
    if tuple(flow_prev.shape) != (total, H, W, 2) or tuple(flow_next.shape) != (total, H, W, 2):
        raise ValueError("flow_prev and flow_next must be [total,H,W,2] like masks [total,H,W]")
    lens = np.asarray(seq_lens, dtype=np.int64).reshape(-1)
    if lens.sum() != total:
        raise ValueError("seq_lens must sum to the {} frames of masks".format(total))
    first, length = check_sequence_tables(np.concatenate([[0], np.cumsum(lens)[:-1]]), lens, total)  # before the device is touched
    d_first, d_len = upload_tables([first, length], masks.device)
    avg_f, avg_b = torch.empty_like(masks), torch.empty_like(masks)
    ws = workspace(lib.udet_post_propagate_workspace_bytes(total, len(first)), 16, masks.device)
    check(lib.udet_post_propagate_sequences(masks.data_ptr(), flow_prev.data_ptr(), flow_next.data_ptr(), len(first), d_first.data_ptr(),
                                            d_len.data_ptr(), total, H, W, float(np.float32(1 - w_r)), float(np.float32(w_r)),
                                            avg_f.data_ptr(), avg_b.data_ptr(), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream(masks.device).cuda_stream))
    return avg_f, avg_b


def _propagate_batched(seq_masks, seq_images, flow_fn, w_r, flow_batch):
    """propagate(flow_batch=...) for a list of sequences: every flow of every sequence through flow_fn.batch (2 (n - 1) pairs per
    sequence of n frames), then one propagate_sequences call.  Returns [(running_avg_f, running_avg_b), ...], one pair of lists per
    sequence."""
    if not hasattr(flow_fn, "batch"):
        raise ValueError("flow_batch needs a flow_fn with a batch(imgs_from, imgs_to, batch) method (PWCFlow)")
    masks = [_as_mask(m) for ms in seq_masks for m in ms]
    lens = [len(ms) for ms in seq_masks]
    if any(len(ms) != len(im) or not len(ms) for ms, im in zip(seq_masks, seq_images)):
        raise ValueError("one frame per mask, and at least one mask per sequence")
    masks = torch.stack(masks, 0).contiguous()
    total, H, W = masks.shape
    a, b, slot = [], [], []  # pair i: flow from a[i] to b[i], stored at (direction, frame) = slot[i]
    base = 0
    for im in seq_images:
        n = len(im)
        for k in range(1, n):
            a.append(im[k]), b.append(im[k - 1]), slot.append(base + k)
        for k in range(n - 1):
            a.append(im[k]), b.append(im[k + 1]), slot.append(total + base + k)
        base += n
    flows = torch.zeros((2 * total, H, W, 2), dtype=torch.float32, device=masks.device)
    if slot:
        flows[torch.as_tensor(slot, device=masks.device)] = flow_fn.batch(a, b, int(flow_batch))
    avg_f, avg_b = propagate_sequences(masks, flows[:total], flows[total:], lens, w_r)
    out, base = [], 0
    for n in lens:
        out.append((list(avg_f[base:base + n]), list(avg_b[base:base + n])))
        base += n
    return out


def propagate(pred_masks, images_u8, flow_fn, w_r=0.85, flow_batch=None):
    """Moving average of a sequence's masks along the optical flow, forward and backward (:127-231).  pred_masks: list of [H,W]
    soft masks, images_u8: list of [H,W,3] uint8 frames, flow_fn(I_a, I_b) -> (u, v) field used as in the reference's calls
    (forward pass: flow_fn(I_k, I_{k-1}); backward pass: flow_fn(I_k, I_{k+1})).  Returns (running_avg_f, running_avg_b) lists.
    flow_batch None: one flow_fn call and four launches per frame and direction.  An integer: all flows through flow_fn.batch, that
    many pairs per network call, then one propagate_sequences call."""
    if flow_batch is not None:
        return _propagate_batched([pred_masks], [images_u8], flow_fn, w_r, flow_batch)[0]
    n = len(pred_masks)
    masks = [_as_mask(m) for m in pred_masks]
    fwd, bwd = [None] * n, [None] * n
    ra = masks[0]
    fwd[0] = ra
    for k in range(1, n):
        ra = propagate_step(ra, masks[k - 1], flow_fn(images_u8[k], images_u8[k - 1]), w_r)
        fwd[k] = ra
    ra = masks[n - 1]
    bwd[n - 1] = ra
    for k in range(n - 2, -1, -1):
        ra = propagate_step(ra, masks[k + 1], flow_fn(images_u8[k], images_u8[k + 1]), w_r)
        bwd[k] = ra
    return fwd, bwd


# --------------------------------------------------------------------------------------------------------------- CRF ----
def select_candidate(pred_mask, pred_f, pred_b, gt_mask):
    """crf_refine.py:40-50: the candidate with the largest object score sum(p * gt) / (sum(p) + 1e-8)."""
    gt = _dev(gt_mask, torch.float32)

    def objscore(p):
        p = _dev(p, torch.float32)
        return float((p * gt).sum() / (p.sum() + 1e-8))
    m, f, b = objscore(pred_mask), objscore(pred_f), objscore(pred_b)
    if m >= f and m >= b:
        return pred_mask, 0
    if f >= m and f >= b:
        return pred_f, 1
    return pred_b, 2


def select_unary_batch(pred, avg_f, avg_b, gt, gauss_k=0.1):
    """select_candidate and the unary of refine (crf_refine.py:40-52, :113-121) for n same-size frames in one call of
    udet_post_select_unary (two launches, no host round trip).  pred, avg_f, avg_b, gt: device float32 [n,H,W].  Returns (choice int32 [n],
    scores float64 [n,3] = the object scores of (pred, avg_f, avg_b), soft float32 [n,H,W] = the chosen candidate, unary float32
    [2, n*H*W] with frame i at element i*H*W: what dense_crf_ragged takes with offsets i*H*W), all on the device.  Only the identity
    Gaussian (int(4 gauss_k + 0.5) == 0, the reference's 0.1): ValueError otherwise -- run_crf then keeps the per-frame path."""
    if int(4.0 * float(gauss_k) + 0.5) != 0:
        raise ValueError("select_unary_batch covers gauss_k with int(4 gauss_k + 0.5) == 0 only")
    for t, name in ((pred, "pred"), (avg_f, "avg_f"), (avg_b, "avg_b"), (gt, "gt")):
        if require_tensor(t, name + " [n,H,W]", torch.float32, 3).shape != pred.shape:
            raise ValueError("pred, avg_f, avg_b and gt must be of one shape [n,H,W]")
    n, H, W = (int(v) for v in pred.shape)
    dev = pred.device
    choice = torch.empty(n, dtype=torch.int32, device=dev)
    scores = torch.empty((n, 3), dtype=torch.float64, device=dev)
    soft = torch.empty_like(pred)
    unary = torch.empty((2, n * H * W), dtype=torch.float32, device=dev)
    check(lib.udet_post_select_unary(pred.data_ptr(), avg_f.data_ptr(), avg_b.data_ptr(), gt.data_ptr(), n, H * W, choice.data_ptr(),
                                     scores.data_ptr(), soft.data_ptr(), unary.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return choice, scores, soft, unary


def gaussian_filter(x, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter(x, sigma) (mode='reflect') on the device, float64."""
    t = _dev(x, torch.float64)
    r = int(truncate * float(sigma) + 0.5)
    if r == 0:
        return t.clone()
    k = np.exp(-0.5 / (sigma * sigma) * np.arange(-r, r + 1) ** 2)
    k = torch.from_numpy(k / k.sum()).cuda()
    H, W = t.shape
    for ax in (0, 1):
        out = torch.empty_like(t)
        check(lib.udet_post_gauss1d(t.data_ptr(), out.data_ptr(), H, W, k.data_ptr(), r, ax, _stream()))
        t = out
    return t


def dense_crf(unary, image_u8, sxy, srgb, compat, iters=50, radius=None):
    """DenseCRF2D + setUnaryEnergy + addPairwiseBilateral + inference(iters) (crf_refine.py:111-130) -> Q device float32 [2,H,W]."""
    un = _dev(unary, torch.float32)
    img = _dev(image_u8, torch.uint8)
    _, H, W = un.shape
    R = int(math.ceil(3.0 * sxy)) if radius is None else int(radius)
    q = torch.empty_like(un)
    ws = workspace(lib.udet_post_crf_workspace_bytes(H, W), 16, un.device)
    check(lib.udet_post_dense_crf(un.data_ptr(), img.data_ptr(), H, W, sxy, srgb, compat, iters, R, q.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _stream()))
    return q


def refine(mask, image, gk, sxy, srgb, compat, gtmask, iters=50, radius=None):
    """crf_refine.py:110-138 -> (new_mask numpy float32 [H,W] in {0,1}, IoU against gt > 0.1)."""
    U = gaussian_filter(mask, gk)
    U = U / (U.max() + 1e-8)
    U = torch.clamp(U, 1e-6, 1.0 - 1e-6)
    unary = (-torch.log(torch.stack([1.0 - U, U], 0))).float()
    Q = dense_crf(unary, image, sxy, srgb, compat, iters, radius)
    new_mask = (Q[1] > Q[0]).float().cpu().numpy()  # np.argmax(Q, axis=0): label 1 only where strictly larger
    gt, bm = np.asarray(gtmask) > 0.1, new_mask > 0.1
    return new_mask, np.float32(np.sum(gt & bm)) / np.float32(np.sum(gt | bm))


# ------------------------------------------------------------------------------------- CRF at native resolution ----
def default_radius(sxy):
    """The window radius of the truncated Gaussian: ceil(3 sxy)."""
    return int(math.ceil(3.0 * float(sxy)))


def unary_table(amax):
    """crf_refine.py:93-97,113-121 with the reference's gauss_k = 0.1 (a Gaussian of radius int(4 gauss_k + 0.5) = 0: the identity) as
    a function of the restored byte: the soft value is byte / (amax + 1e-8), its maximum amax / (amax + 1e-8), so
    U = soft / (max + 1e-8), clipped to [1e-6, 1 - 1e-6], and the energies -log(1 - U), -log(U).  amax: int [n] (the largest byte of
    each sample) -> float32 [n,2,256], computed in float64 with numpy like oracle_post.unary_from_mask.  amax = 0 (a constant mask):
    U = 1e-6 everywhere."""
    a = np.asarray(amax, dtype=np.float64).reshape(-1, 1)
    soft = np.arange(256, dtype=np.float64)[None, :] / (a + 1e-8)
    U = soft / (a / (a + 1e-8) + 1e-8)
    U = np.clip(U, 1e-6, 1.0 - 1e-6)
    return np.ascontiguousarray(np.float32(-np.log(np.stack([1.0 - U, U], 1))))


CRF_MAX_SAMPLES = 65535  # a grid dimension of udet_dense_crf_ragged / udet_crf_unary_lookup


def unary_from_restored(data, offsets, hw, amax, gauss_k=0.1):
    """The unary energies of refine (crf_refine.py:113-121) for the packed restored bytes `data` (1-D uint8 device tensor in the layout
    offsets / hw -- host arrays, or a PackedLayout with hw=None; amax [n]: each sample's largest byte, device or host) -> device
    float32 [2,total], packed the same way (elements between samples are 0).
    A Gaussian of radius 0 (int(4 gauss_k + 0.5) == 0, the reference's 0.1): a 256-entry table
    per sample (unary_table) and one lookup launch for the batch, bit-equal to oracle_post.unary_from_mask of the float64 soft mask.
    A wider Gaussian goes through gaussian_filter per sample (slow, correct, not what the reference uses)."""
    require_tensor(data, "data (packed samples)", torch.uint8, 1)
    total, dev = int(data.numel()), data.device
    layout = as_layout(offsets, hw, total, max_samples=CRF_MAX_SAMPLES)  # raw tables: validated before the device is touched
    am = (amax.cpu().numpy() if isinstance(amax, torch.Tensor) else np.asarray(amax)).reshape(-1).astype(np.int64)
    if len(am) != layout.n or (am < 0).any() or (am > 255).any():
        raise ValueError("one amax in 0..255 per sample")
    unary = torch.zeros((2, total), dtype=torch.float32, device=dev)
    if int(4.0 * float(gauss_k) + 0.5) == 0:
        table = torch.from_numpy(unary_table(am)).to(dev)
        d_off, d_hw = layout.device_tables(dev)
        check(lib.udet_crf_unary_lookup(data.data_ptr(), table.data_ptr(), layout.n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h,
                                        layout.max_w, total, unary.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return unary
    for i in range(layout.n):
        U = gaussian_filter(layout.view(data, i).double() / (float(am[i]) + 1e-8), gauss_k)
        U = torch.clamp(U / (U.max() + 1e-8), 1e-6, 1.0 - 1e-6)
        o = int(layout.offsets[i])
        unary[:, o:o + U.numel()] = (-torch.log(torch.stack([1.0 - U, U], 0))).float().view(2, -1)
    return unary


def dense_crf_ragged(unary, images, offsets, hw, sxy, srgb, compat, iters=50, radius=None, want_q=True, want_labels=True, q_out=None,
                     labels_out=None):
    """The dense CRF of dense_crf on n frames of their own sizes in one call of udet_dense_crf_ragged (iters + 2 launches whatever
    n is).  unary: device float32 [2,total] (the energies of label 0 / 1), images: device uint8 [3 * total] (rgb), both in the layout
    offsets / hw of `total` elements (host arrays [n] / [n,2], or a PackedLayout with hw=None).  radius None: ceil(3 sxy).
    Returns (q1, labels): the marginal of label 1 (device float32 [total]) and the label (device uint8 [total], 1 where Q1 > Q0), each
    None when not wanted; elements between the samples are not written (q_out / labels_out: caller-owned buffers of `total`
    elements, else fresh zeroed ones).  Raw tables are validated on the host before anything is launched (ValueError)."""
    if require_tensor(unary, "unary [2,total]", torch.float32, 2).shape[0] != 2:
        raise ValueError("unary must be [2,total]")
    total, dev = int(unary.shape[1]), unary.device
    require_tensor(images, "images (rgb, packed like unary)", torch.uint8, None, 3 * total, dev)
    if not (want_q or want_labels):
        raise ValueError("at least one of want_q and want_labels")
    for buf, dt, name in ((q_out, torch.float32, "q_out"), (labels_out, torch.uint8, "labels_out")):
        if buf is not None:
            require_tensor(buf, name, dt, 1, total, dev)
    layout = as_layout(offsets, hw, total, max_samples=CRF_MAX_SAMPLES)
    d_off, d_hw = layout.device_tables(dev)
    R = default_radius(sxy) if radius is None else int(radius)
    q1 = (torch.zeros(total, dtype=torch.float32, device=dev) if q_out is None else q_out) if want_q else None
    labels = (torch.zeros(total, dtype=torch.uint8, device=dev) if labels_out is None else labels_out) if want_labels else None
    ws = workspace(lib.udet_dense_crf_workspace_bytes(total, layout.n), 16, dev)
    check(lib.udet_dense_crf_ragged(unary.data_ptr(), images.data_ptr(), layout.n, d_off.data_ptr(), d_hw.data_ptr(), layout.max_h,
                                    layout.max_w, total, float(sxy), float(srgb), float(compat), int(iters), R,
                                    None if q1 is None else q1.data_ptr(), None if labels is None else labels.data_ptr(), ws.data_ptr(),
                                    ws.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return q1, labels


def run_crf_original_resolution(path_soft, frame_lists, sxy, srgb, scomp, gauss_k, out_path="./post_processed_davis_original", **kwargs):
    """crf_refine.run_crf_original_resolution (:65-108) over the folder run_crf wrote: soft_mask of every result_<k>.mat restored to
    its frame's own size, refined there by the dense CRF on the untouched frame, scored and exported.  frame_lists ({category:
    [(image, annotation), ...]}, native_results.frame_lists_from_reader) stands for the reference's path_img / path_gt.  A thin call
    of native_results.restore_results_dir (its other arguments -- component, batch, gt_rule, ... -- ride along in kwargs; crf_iters /
    crf_radius: the iterations (50) and the window radius (ceil(3 sxy))); returns what it returns, native_eval.json's content."""
    from .native_results import restore_results_dir
    crf = {"sxy": sxy, "srgb": srgb, "compat": scomp, "gauss_k": gauss_k, "iters": kwargs.pop("crf_iters", 50),
           "radius": kwargs.pop("crf_radius", None)}
    kwargs.setdefault("mask_key", "soft_mask")
    return restore_results_dir(path_soft, frame_lists, out_path, crf=crf, **kwargs)


# ----------------------------------------------------------------------------------------------------- file drivers ----
def _save_soft(out_dir, masks, imgs, gts, fwd, bwd):
    """result_<k>.mat of one sequence as buffer_to_soft_score writes them."""
    import scipy.io as sio
    for k in range(len(masks)):
        sio.savemat(os.path.join(out_dir, "result_%d.mat" % (k + 1)),
                    {"pred_mask": masks[k].cpu().numpy(), "img1": imgs[k], "gt_mask": gts[k],
                     "running_avg_f": fwd[k].cpu().numpy(), "running_avg_b": bwd[k].cpu().numpy()})


def buffer_to_soft_score(buffer_path, out_path, seq_names, seq_num, max_shift=2, base_crop=90.0, dprefix="davis_shift", flow_fn=None,
                         flow_batch=None, score_batch=None):
    """generate_soft_score_from_buffer.buffer_to_soft_score over the result_<k>.mat buffers test_generator_ensemble writes
    (evaluation.evaluate_ensemble), followed by propagate(); writes result_<k>.mat with pred_mask / img1 / gt_mask /
    running_avg_f / running_avg_b like the reference (:91-93, :148, :184, :199, :229).  flow_batch (None: propagate() per sequence as
    it is read): an integer computes the soft scores of the whole folder first and propagates all its sequences in one call.
    score_batch (None: a soft_score call per frame): an integer takes a sequence's frames in groups of that many -- one host buffer, one
    upload and one soft_score_batch call per group, the last group of a sequence shorter; the same files, keys and dtypes.  The frame is
    the masks' own size (the reference's 192 x 384)."""
    import scipy.io as sio
    crops = list(range(85, 101, 5))
    if score_batch is not None and int(score_batch) < 1:
        raise ValueError("buffer_to_soft_score: score_batch must be None or at least 1")
    held = []  # flow_batch: (out_dir, masks, imgs, gts) of every sequence until the one propagation
    for name, num in zip(seq_names, seq_num):
        out_dir = os.path.join(out_path, name)
        os.makedirs(out_dir, exist_ok=True)
        print(out_dir)
        masks, imgs, gts = [], [], []
        group = None  # score_batch: the host buffer [frames, 2, shifts, crops, H, W] of the group being read
        for k in range(1, num + 1):
            pb, pf, r_f1 = [], [], None
            for shift in range(1, max_shift + 1):
                r_b = sio.loadmat(os.path.join(buffer_path, "%s_%d" % (dprefix, -shift), name, "result_%d.mat" % k))
                r_f = sio.loadmat(os.path.join(buffer_path, "%s_%d" % (dprefix, shift), name, "result_%d.mat" % k))
                pb.append([np.squeeze(r_b["pred_mask_%03d" % c]) for c in crops])
                pf.append([np.squeeze(r_f["pred_mask_%03d" % c]) for c in crops])
                if shift == 1:
                    r_f1 = r_f
            if score_batch is None:
                masks.append(soft_score(pb, pf, crops, base_crop, pb[0][0].shape))
            else:
                at = (k - 1) % int(score_batch)
                if at == 0:
                    group = np.empty((min(int(score_batch), num - k + 1), 2, max_shift, len(crops)) + pb[0][0].shape, np.float32)
                group[at, 0], group[at, 1] = np.asarray(pb), np.asarray(pf)
                if at == len(group) - 1:
                    masks.extend(soft_score_batch(group, crops, base_crop))
            imgs.append(((r_f1["img_1_%03d" % int(base_crop)] + 0.5) * 255).astype("uint8"))
            gts.append(r_f1["gt_mask_%03d" % int(base_crop)])
        if flow_batch is not None:
            held.append((out_dir, masks, imgs, gts))
            continue
        _save_soft(out_dir, masks, imgs, gts, *propagate(masks, imgs, flow_fn or PWCFlow()))
    if held:
        avgs = _propagate_batched([h[1] for h in held], [h[2] for h in held], flow_fn or PWCFlow(), 0.85, flow_batch)
        for (out_dir, masks, imgs, gts), (fwd, bwd) in zip(held, avgs):
            _save_soft(out_dir, masks, imgs, gts, fwd, bwd)


def _run_crf_group(frames, sxy, srgb, scomp, gauss_k, iters, radius):
    """The device part of run_crf(batch=...) for a group of same-size frames [(pred_mask, running_avg_f, running_avg_b, gt_mask float32
    [H,W], img1 uint8 [H,W,3]), ...]: one upload, select_unary_batch, one dense_crf_ragged call, the IoU's integer counts on the
    device, one copy back -> (soft float32 [n,H,W], labels uint8 [n,H,W], intersection int64 [n], union int64 [n]) on the host."""
    n, (H, W) = len(frames), frames[0][0].shape
    hw = H * W
    buf = np.empty(16 * n * hw + 3 * n * hw, np.uint8)
    fl = buf[:16 * n * hw].view(np.float32).reshape(4, n, hw)
    im = buf[16 * n * hw:].reshape(n, hw * 3)
    for i, fr in enumerate(frames):
        for c in range(4):
            fl[c, i] = fr[c].reshape(-1)
        im[i] = np.asarray(fr[4], np.uint8).reshape(-1)
    d = torch.from_numpy(buf).cuda()
    dfl = d[:16 * n * hw].view(torch.float32).view(4, n, H, W)
    choice, _, soft, unary = select_unary_batch(dfl[0], dfl[1], dfl[2], dfl[3], gauss_k)
    _, labels = dense_crf_ragged(unary, d[16 * n * hw:], PackedLayout.packed([(H, W)] * n), None, sxy, srgb, scomp, iters, radius, want_q=False)
    gt, bm = dfl[3].reshape(n, hw) > 0.1, labels.view(n, hw) > 0
    counts = torch.stack([(gt & bm).sum(1), (gt | bm).sum(1)], 0)  # int64 [2,n]: exact
    back = torch.cat([soft.reshape(-1).view(torch.uint8), counts.reshape(-1).view(torch.uint8), labels]).cpu().numpy()
    soft_h = back[:4 * n * hw].view(np.float32).reshape(n, H, W)
    cnt = back[4 * n * hw:4 * n * hw + 16 * n].view(np.int64).reshape(2, n)
    return soft_h, back[4 * n * hw + 16 * n:].reshape(n, H, W), cnt[0], cnt[1]


def run_crf(path_soft, sxy, srgb, scomp, gauss_k, out_path="./post_processed_davis", batch=None, crf_iters=50, crf_radius=None):
    """crf_refine.run_crf (:9-59) over the soft-score folder; returns the average IoU.  crf_iters / crf_radius: the mean-field
    iterations and the window radius of the kernel (None: ceil(3 sxy)).  batch None: a frame at a time (select_candidate + refine).  An
    integer: the frames of a sequence in groups of that many -- one upload, select_unary_batch, one dense_crf_ragged call and one copy back
    per group (_run_crf_group); the same files, keys and dtypes, the same return value.  A Gaussian wider than the identity (int(4 gauss_k
    + 0.5) > 0, not what the reference uses) keeps the per-frame path."""
    import scipy.io as sio
    sum_iou, total = 0.0, 0.0
    if batch is not None and int(batch) < 1:
        raise ValueError("run_crf: batch must be None or at least 1")
    if batch is not None and int(4.0 * float(gauss_k) + 0.5) != 0:
        batch = None

    def load(seq_path, k):
        result = sio.loadmat(os.path.join(seq_path, "result_%d.mat" % (k + 1)))
        return tuple(np.float32(np.squeeze(result[n])) for n in ("pred_mask", "running_avg_f", "running_avg_b", "gt_mask")) + (result["img1"],)
    for seq in os.listdir(path_soft):
        seq_path = os.path.join(path_soft, seq)
        seq_len = len([n for n in os.listdir(seq_path) if n.endswith(".mat")])
        out_dir = os.path.join(out_path, seq)
        os.makedirs(out_dir, exist_ok=True)
        print(out_dir)
        group = 1 if batch is None else int(batch)
        for k0 in range(0, seq_len, group):
            ks = range(k0, min(seq_len, k0 + group))
            frames = [load(seq_path, k) for k in ks]
            if batch is None:
                pm, pf, pb, gt, img = frames[0]
                mask, _ = select_candidate(pm, pf, pb, gt)
                new_mask, iou = refine(mask, img, gauss_k, sxy, srgb, scomp, gt, crf_iters, crf_radius)
                soft, masks, ious = [mask], [new_mask], [iou]
            else:
                soft, labels, inter, union = _run_crf_group(frames, sxy, srgb, scomp, gauss_k, crf_iters, crf_radius)
                masks, ious = labels.astype(np.float32), [np.float32(a) / np.float32(b) for a, b in zip(inter, union)]
            for i, k in enumerate(ks):
                total += 1.0
                sio.savemat(os.path.join(out_dir, "result_%d.mat" % (k + 1)), {"gt_mask": frames[i][3], "soft_mask": soft[i], "mask": masks[i]})
                sum_iou += ious[i]
    return sum_iou / total
