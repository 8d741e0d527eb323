"""Evaluation tail of the hot path ("next" row N2 of SURVEY.md section 8f), backed by udet_mask_stats.

Mirrors, with the reference's names and return contracts:
  compute_boundary_score(segmentation)                  models/utils/general_utils.py:122-138
  disambiguate_forw_back(pred_masks, threshold=0.1)     models/utils/general_utils.py:100-110
  compute_all_IoU(pred_masks, gt_masks, threshold=0.1)  models/utils/general_utils.py:112-116 (+ tf_iou_computation :89-98)
  compute_IoU(gt_mask, pred_mask_f, threshold=0.1)      test_generator.py:19-35
  compute_mae(gt_mask, pred_mask_f)                     test_generator.py:38-40
  evaluate_masks(learner, ...)                          the aggregation / report of test_generator.py:43-130

The batch functions take device tensors [B,H,W,1]; one kernel pass produces every per-sample sum both IoU variants and
the MAE need (exact counts, double accumulation), the few scalar operations that remain run on the host.

Not in the reference (its authors ran the external DAVIS toolkit): the DAVIS-2016 benchmark measures, backed by
udet_boundary_stats -- boundary_stats / compute_boundary_f / f_from_counts (contour accuracy F), davis_statistics (mean, recall,
decay), evaluate_batch_davis, evaluate_masks(davis_metrics=True) and evaluate_results_dir (the `davis_eval` subcommand)."""
from __future__ import annotations

import os

import numpy as np
import torch

from ._ffi import c_f, c_i, c_p, check, lib

lib.udet_mask_stats.restype = c_i
lib.udet_mask_stats.argtypes = [c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_p, c_p]
lib.udet_boundary_stats.restype = c_i
lib.udet_boundary_stats.argtypes = [c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_i, c_p, c_p, c_p, c_p]

MASK_THRESHOLD = 0.6  # test_generator.py:16 / general_utils.py:101


def _check_masks(pred_masks, gt_masks):
    for t, name in ((pred_masks, "pred_masks"), (gt_masks, "gt_masks")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 CUDA(HIP) tensor")
    if pred_masks.shape != gt_masks.shape or pred_masks.dim() != 4 or pred_masks.shape[-1] != 1:
        raise ValueError("masks must both be [B,H,W,1]")


def mask_stats_device(pred_masks: torch.Tensor, gt_masks: torch.Tensor, threshold: float = 0.1, gt_threshold: float = 0.0) -> torch.Tensor:
    """mask_stats, left on the device ([B,8] float64 tensor): what boundary_stats / visualize take as `stats`."""
    _check_masks(pred_masks, gt_masks)
    b, h, w, _ = pred_masks.shape
    out = torch.empty((b, 8), dtype=torch.float64, device=pred_masks.device)
    check(lib.udet_mask_stats(pred_masks.data_ptr(), gt_masks.data_ptr(), b, h, w, threshold, gt_threshold, out.data_ptr(),
                              torch.cuda.current_stream().cuda_stream))
    return out


def mask_stats(pred_masks: torch.Tensor, gt_masks: torch.Tensor, threshold: float = 0.1, gt_threshold: float = 0.0) -> np.ndarray:
    """[B,8] float64: border sum, |pred|, |gt|, |pred&gt|, sum pred|gt-1|, sum (1-pred)|gt|, sum (1-pred)|gt-1|, sum pred|gt|."""
    return mask_stats_device(pred_masks, gt_masks, threshold, gt_threshold).cpu().numpy()


def _border_score(stats, h, w):
    return stats[:, 0] / float(2 * 2 * w + 2 * 2 * h)


def compute_boundary_score(segmentation) -> float:
    """Fraction of the four 2-pixel image borders the (boolean / 0-1) mask covers; >= 0.6 means background."""
    seg = torch.as_tensor(np.asarray(segmentation, dtype=np.float32)).reshape(1, segmentation.shape[0], segmentation.shape[1], 1)
    st = mask_stats(seg.cuda().contiguous(), torch.zeros_like(seg).cuda(), threshold=0.5)
    return float(_border_score(st, seg.shape[1], seg.shape[2])[0])


def disambiguate_forw_back(pred_masks: torch.Tensor, threshold: float = 0.1) -> torch.Tensor:
    """Binary masks, complemented per sample when they cover the image borders (score >= 0.6)."""
    b, h, w, _ = pred_masks.shape
    st = mask_stats(pred_masks, torch.zeros_like(pred_masks), threshold)
    fg = torch.as_tensor(_border_score(st, h, w) < MASK_THRESHOLD, device=pred_masks.device).view(-1, 1, 1, 1)
    binm = (pred_masks > threshold).to(torch.float32)
    return torch.where(fg, binm, 1.0 - binm)


def _iou_terms(st, hw, flip):
    n_pred, n_gt, inter = st[:, 1], st[:, 2], st[:, 3]
    inter_c, n_pred_c = n_gt - inter, hw - n_pred
    i = np.where(flip, inter_c, inter)
    u = np.where(flip, n_pred_c + n_gt - inter_c, n_pred + n_gt - inter)
    ann = np.where(flip, n_pred_c, n_pred)
    return i, u, ann


def compute_all_IoU(pred_masks: torch.Tensor, gt_masks: torch.Tensor, threshold: float = 0.1) -> np.ndarray:
    """The validation IoU of the training graph (adversarial_learner.py:135-139): gt > 0.01, |and| / (|or| + 1e-8)."""
    b, h, w, _ = pred_masks.shape
    st = mask_stats(pred_masks, gt_masks, threshold, 0.01)
    flip = _border_score(st, h, w) >= MASK_THRESHOLD
    i, u, _ = _iou_terms(st, float(h * w), flip)
    return i / (u + 1e-8)


def _batch_scores(st, h, w):
    """Host part of evaluate_batch from the [B,8] sums: (iou, mae, flip, intersection, union)."""
    hw = float(h * w)
    flip = _border_score(st, h, w) >= MASK_THRESHOLD
    i, u, ann = _iou_terms(st, hw, flip)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where((ann == 0) & (st[:, 2] == 0), 1.0, i / u.astype(np.float32))
    mae = np.where(flip, st[:, 6] + st[:, 7], st[:, 4] + st[:, 5]) / hw
    return iou, mae, flip, i, u


def evaluate_batch(gt_masks: torch.Tensor, pred_masks: torch.Tensor, threshold: float = 0.1):
    """Per sample (iou, mae, flipped) with the semantics of test_generator.py compute_IoU / compute_mae:
    gt cast to bool for the IoU (1.0 when annotation and gt are both empty), MAE = mean |gt - annotation|."""
    b, h, w, _ = pred_masks.shape
    st = mask_stats(pred_masks, gt_masks, threshold, 0.0)
    return _batch_scores(st, h, w)[:3]


def compute_IoU(gt_mask, pred_mask_f, threshold: float = 0.1):
    """Single-image form of test_generator.py:19-35: returns (iou, annotation) -- or a bare 1 when both are empty."""
    g = torch.as_tensor(np.asarray(gt_mask, dtype=np.float32)).reshape(1, *np.asarray(gt_mask).shape[:2], 1).cuda().contiguous()
    p = torch.as_tensor(np.asarray(pred_mask_f, dtype=np.float32)).reshape(g.shape).cuda().contiguous()
    iou, _, flip = evaluate_batch(g, p, threshold)
    pred = np.asarray(pred_mask_f) > threshold
    annotation = np.logical_not(pred) if flip[0] else pred
    if not annotation.any() and not np.asarray(gt_mask).astype(bool).any():
        return 1
    return float(iou[0]), annotation


def compute_mae(gt_mask, pred_mask_f) -> float:
    return float(np.mean(np.abs(np.asarray(gt_mask, dtype=np.float64) - np.asarray(pred_mask_f, dtype=np.float64))))


# ---------------------------------------------------------------------------------------------------------------------------
# DAVIS-2016 benchmark measures: region similarity J, contour accuracy F, each as mean / recall / decay per sequence.
# A restatement of the published measures (Perazzi et al., CVPR 2016: db_eval_boundary, db_statistics); the reference reports them
# through the external DAVIS toolkit and has no code for them.  Definitions: include/udet.h (udet_boundary_stats), DESIGN.md.
# ---------------------------------------------------------------------------------------------------------------------------
BOUND_TH = 0.008  # the toolkit's default: the matching radius as a fraction of the image diagonal


def boundary_radius(h: int, w: int, bound_th: float = BOUND_TH) -> int:
    """bound_th itself when >= 1 (pixels), else ceil(bound_th * image diagonal): 4 at 192x384, 8 at 480x854, 36 at 2160x3840."""
    return int(bound_th) if bound_th >= 1 else int(np.ceil(bound_th * np.sqrt(float(h) * h + float(w) * w)))


def boundary_stats(pred_masks: torch.Tensor, gt_masks: torch.Tensor, bound_th: float = BOUND_TH, threshold: float = 0.1,
                   gt_threshold: float = 0.0, stats=None, return_maps: bool = False):
    """[B,4] int64 = (n_fg, n_gt, fg_match, gt_match): boundary pixels of pred > threshold and of gt > gt_threshold, and how many of
    each lie within the radius of the other's boundary (udet_boundary_stats, one launch).  `stats`: the [B,8] tensor of
    mask_stats_device for the same prediction -- a sample whose mask hugs the image borders is then complemented on the device
    (disambiguate_forw_back); None: never.  return_maps: also the two boundary maps, uint8 [B,H,W] device tensors."""
    _check_masks(pred_masks, gt_masks)
    b, h, w, _ = pred_masks.shape
    dev = pred_masks.device
    if stats is not None:
        stats = torch.as_tensor(stats, dtype=torch.float64).to(dev).contiguous()
        if tuple(stats.shape) != (b, 8):
            raise ValueError("stats must be [B,8] (mask_stats_device)")
    counts = torch.empty((b, 4), dtype=torch.int64, device=dev)  # the library writes uint64; the counts are far below 2^63
    maps = [torch.empty((b, h, w), dtype=torch.uint8, device=dev) for _ in range(2)] if return_maps else None
    check(lib.udet_boundary_stats(pred_masks.data_ptr(), gt_masks.data_ptr(), None if stats is None else stats.data_ptr(), b, h, w,
                                  threshold, gt_threshold, boundary_radius(h, w, bound_th), counts.data_ptr(),
                                  maps[0].data_ptr() if maps else None, maps[1].data_ptr() if maps else None,
                                  torch.cuda.current_stream().cuda_stream))
    c = counts.cpu().numpy()
    return (c, maps[0], maps[1]) if return_maps else c


def f_from_counts(counts):
    """(F, precision, recall) in float64 from [...,4] counts (n_fg, n_gt, fg_match, gt_match): an empty prediction boundary has
    precision 1, an empty ground-truth boundary recall 1 (and the other one 0 unless both are empty); F = 2pr / (p + r), 0 when
    p + r = 0."""
    c = np.asarray(counts)
    n_fg, n_gt, m_fg, m_gt = (c[..., k].astype(np.float64) for k in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(n_fg > 0, np.where(n_gt > 0, m_fg / n_fg, 0.0), 1.0)
        r = np.where(n_gt > 0, np.where(n_fg > 0, m_gt / n_gt, 0.0), 1.0)
        f = np.where(p + r == 0, 0.0, 2 * p * r / (p + r))
    return f, p, r


def compute_boundary_f(gt_mask, pred_mask_f, bound_th: float = BOUND_TH, threshold: float = 0.1):
    """Single-image form: (F, precision, recall) of pred_mask_f > threshold against gt_mask cast to bool (no fg/bg flip)."""
    g = torch.as_tensor(np.asarray(gt_mask, dtype=np.float32)).reshape(1, *np.asarray(gt_mask).shape[:2], 1).cuda().contiguous()
    p = torch.as_tensor(np.asarray(pred_mask_f, dtype=np.float32)).reshape(g.shape).cuda().contiguous()
    f, pr, rc = f_from_counts(boundary_stats(p, g, bound_th, threshold, 0.0))
    return float(f[0]), float(pr[0]), float(rc[0])


def _nanmean(x):
    x = np.asarray(x, dtype=np.float64)
    x = x[~np.isnan(x)]
    return float(x.mean()) if x.size else float("nan")


def davis_statistics(values, skip_ends: bool = True):
    """{mean, recall, decay} of a sequence's per-frame J or F (db_statistics): mean = nanmean(v), recall = mean(v > 0.5), decay =
    nanmean of the first minus nanmean of the last of four bins bounded by ids = round(linspace(1, len(v), 5) + 1e-10) - 1 (bin i =
    v[ids[i] : ids[i+1] + 1]).  skip_ends: the DAVIS-2016 protocol leaves the first and the last frame out.  NaN frames are ignored
    by the means (in the recall they count as not recalled, as in the formula); an empty list gives NaN, never an exception."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if skip_ends:
        v = v[1:-1]
    ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.int64)
    bins = [v[max(ids[i], 0):max(ids[i + 1] + 1, 0)] for i in range(4)]
    return {"mean": _nanmean(v), "recall": float(np.mean(v > 0.5)) if v.size else float("nan"),
            "decay": _nanmean(bins[0]) - _nanmean(bins[3])}


def evaluate_batch_davis(gt_masks: torch.Tensor, pred_masks: torch.Tensor, threshold: float = 0.1, bound_th: float = BOUND_TH,
                         disambiguate: bool = True):
    """evaluate_batch plus the DAVIS per-frame measures: (iou, mae, flipped, J, F) from one udet_mask_stats and one
    udet_boundary_stats call; the border statistics that decide the fg/bg flip go from the first to the second on the device.
    J = |fg & gt| / |fg | gt| in float64, 1 when both are empty.  disambiguate=False scores the masks as they are (no flip)."""
    b, h, w, _ = pred_masks.shape
    st_dev = mask_stats_device(pred_masks, gt_masks, threshold, 0.0)
    counts = boundary_stats(pred_masks, gt_masks, bound_th, threshold, 0.0, stats=st_dev if disambiguate else None)
    st = st_dev.cpu().numpy()
    if not disambiguate:
        st[:, 0] = 0.0
    iou, mae, flip, i, u = _batch_scores(st, h, w)
    with np.errstate(divide="ignore", invalid="ignore"):
        j = np.where(u == 0, 1.0, i / u)
    return iou, mae, flip, j, f_from_counts(counts)[0]


def _davis_summary(cat_j, cat_f, skip_ends):
    """Per-category and dataset {J, F: {mean, recall, decay}}; a dataset number is the mean over sequences of that statistic."""
    per = {c: {"J": davis_statistics(cat_j[c], skip_ends), "F": davis_statistics(cat_f[c], skip_ends)} for c in cat_j}
    tot = {m: {k: _nanmean([per[c][m][k] for c in per]) for k in ("mean", "recall", "decay")} for m in ("J", "F")}
    tot["J&F"] = (tot["J"]["mean"] + tot["F"]["mean"]) / 2
    return per, tot


def _print_davis_table(per, tot):
    row = "{:<24s}" + " {:>8s}" * 6
    print(row.format("DAVIS metrics", "J mean", "J recall", "J decay", "F mean", "F recall", "F decay"))
    fmt = lambda d: ["{:.4f}".format(d[m][k]) for m in ("J", "F") for k in ("mean", "recall", "decay")]
    for c in per:
        print(row.format(str(c)[:24], *fmt(per[c])))
    print(row.format("mean over sequences", *fmt(tot)))
    print("J&F mean is {}".format(tot["J&F"]))


def evaluate_results_dir(results_dir, mask_key="pred_mask", threshold=0.5, bound_th=BOUND_TH, skip_ends=True, verbose=True):
    """`davis_eval`: J and F of a folder of <sequence>/result_<k>.mat files (test_generator --generate_visualization,
    post_processing.buffer_to_soft_score, post_processing.run_crf) -- mat[mask_key] > threshold against mat["gt_mask"] cast to bool,
    scored as stored (these masks are already disambiguated).  A sequence's frames go to the device in one batch per frame shape.
    Prints the benchmark table, writes <results_dir>/davis_eval.json and returns its content."""
    import json
    import re
    import scipy.io as sio
    cat_j, cat_f = {}, {}
    for seq in sorted(os.listdir(results_dir)):
        d = os.path.join(results_dir, seq)
        if not os.path.isdir(d):
            continue
        ks = sorted(int(m.group(1)) for m in (re.fullmatch(r"result_(\d+)\.mat", f) for f in os.listdir(d)) if m)
        if not ks:
            continue
        frames = []
        for k in ks:
            mat = sio.loadmat(os.path.join(d, "result_{}.mat".format(k)))
            if mask_key not in mat or "gt_mask" not in mat:
                raise KeyError("{}: result_{}.mat has no {!r} / 'gt_mask'".format(d, k, mask_key))
            frames.append((np.squeeze(mat[mask_key]).astype(np.float32), (np.squeeze(mat["gt_mask"]) != 0).astype(np.float32)))
            if frames[-1][0].ndim != 2 or frames[-1][0].shape != frames[-1][1].shape:
                raise ValueError("{}: result_{}.mat: mask and gt_mask must be 2-D and of one shape".format(d, k))
        j, f = np.empty(len(frames)), np.empty(len(frames))
        for shape in sorted({p.shape for p, _ in frames}):
            idx = [i for i, (p, _) in enumerate(frames) if p.shape == shape]
            pm = torch.as_tensor(np.stack([frames[i][0] for i in idx])[..., None]).cuda().contiguous()
            gm = torch.as_tensor(np.stack([frames[i][1] for i in idx])[..., None]).cuda().contiguous()
            _, _, _, j[idx], f[idx] = evaluate_batch_davis(gm, pm, threshold, bound_th, disambiguate=False)
        cat_j[seq], cat_f[seq] = j.tolist(), f.tolist()
    if not cat_j:
        raise IOError("no <sequence>/result_<k>.mat under {!r}".format(results_dir))
    per, tot = _davis_summary(cat_j, cat_f, skip_ends)
    res = {"mask_key": mask_key, "threshold": threshold, "bound_th": bound_th, "skip_ends": bool(skip_ends),
           "sequences": {c: dict(per[c], frames=len(cat_j[c])) for c in per}, "J": tot["J"], "F": tot["F"], "J&F": tot["J&F"]}
    if verbose:
        _print_davis_table(per, tot)
    with open(os.path.join(results_dir, "davis_eval.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    return res


def _save_frame(d, k, frame_u8, inf, b, flipped):
    """test_generator.py:95-117 for one frame: the overlay PNG and the .mat the offline tools read."""
    import scipy.io as sio
    from PIL import Image
    from .visualize import postprocess_image
    os.makedirs(d, exist_ok=True)
    Image.fromarray(np.ascontiguousarray(frame_u8)).save(os.path.join(d, "frame_{:08d}.png".format(k)))
    pred = np.asarray(inf["gen_masks"][b]) > 0.1
    gt = inf["gt_masks"]
    sio.savemat(os.path.join(d, "result_{}.mat".format(k)),
                {"flow": inf["gt_flow"][b], "img1": postprocess_image(inf["input_image"][b]),
                 "pred_mask": np.logical_not(pred) if flipped else pred,
                 "gt_mask": np.zeros_like(pred, dtype=np.float32) if gt is None else gt[b]})


def evaluate_masks(learner, n_steps=None, verbose=True, save_dir=None, davis_metrics=False, bound_th=BOUND_TH, skip_ends=True):
    """The loop of test_generator.py:_test_masks (:43-130) over learner.inference(): per-category IoU / MAE lists and
    the three reported averages.  `learner` is an AdversarialLearner after setup_inference(config, aug_test=False).
    With `save_dir` (--generate_visualization, :93-117) every frame also leaves <save_dir>/<category>/frame_%08d.png -- the
    image blended with the disambiguated mask at 384 x 640 (visualize.overlay_mask) -- and result_<k>.mat with flow, img1
    (uint8 RGB), pred_mask (the disambiguated mask) and gt_mask; k counts the category's frames from 1.
    davis_metrics (--davis_metrics; not in the reference, which leaves them to the DAVIS toolkit): the result also carries
    category_f (mean boundary F per category), category_davis ({category: {J, F: {mean, recall, decay}}}) and davis ({J, F: the
    mean over categories of each statistic, "J&F": the mean of the two means}), printed as a table after the reference's lines;
    skip_ends leaves the first and last frame of a category out of the statistics (DAVIS-2016 protocol)."""
    cat_iou, cat_mae, cat_j, cat_f = {}, {}, {}, {}
    batch = getattr(learner.config, "batch_size", 1)
    if n_steps is None:
        n_steps = int(np.ceil(learner.test_samples / float(batch)))
    frames = 0
    for _ in range(n_steps):
        try:
            inf = learner.inference(None)
        except StopIteration:
            if verbose:
                print("End of testing dataset")
            break
        pm = torch.as_tensor(np.ascontiguousarray(inf["gen_masks"], dtype=np.float32)).cuda()
        gm = torch.zeros_like(pm) if inf["gt_masks"] is None else \
            torch.as_tensor(np.ascontiguousarray(inf["gt_masks"], dtype=np.float32)).cuda()  # (synthetic data: no annotation)
        if davis_metrics:
            iou, mae, flip, jm, fm = evaluate_batch_davis(gm, pm, bound_th=bound_th)
        else:
            iou, mae, flip = evaluate_batch(gm, pm)
        if save_dir:
            from .visualize import overlay_mask
            img_dev = torch.as_tensor(np.ascontiguousarray(inf["input_image"], dtype=np.float32)).cuda()
            frames_u8 = overlay_mask(img_dev, pm).cpu().numpy()
        for b in range(pm.shape[0]):
            name = inf["img_fname"][b]
            name = name.decode("utf-8") if isinstance(name, (bytes, bytearray)) else str(name)
            parts = name.split("/")
            category = parts[-2] if len(parts) > 1 else "all"
            cat_iou.setdefault(category, []).append(float(iou[b]))
            cat_mae.setdefault(category, []).append(float(mae[b]))
            if davis_metrics:
                cat_j.setdefault(category, []).append(float(jm[b]))
                cat_f.setdefault(category, []).append(float(fm[b]))
            frames += 1
            if save_dir:
                _save_frame(os.path.join(save_dir, category), len(cat_iou[category]), frames_u8[b], inf, b, bool(flip[b]))
    tot_iou = sum(sum(v) for v in cat_iou.values())
    tot_mae = sum(sum(v) for v in cat_mae.values())
    per_cat = [float(np.mean(v)) for v in cat_iou.values()]
    res = {"category_iou": {k: float(np.mean(v)) for k, v in cat_iou.items()},
           "category_mae": {k: float(np.mean(v)) for k, v in cat_mae.items()},
           "dataset_iou": tot_iou / max(frames, 1), "dataset_mae": tot_mae / max(frames, 1),
           "sequence_iou": float(np.mean(per_cat)) if per_cat else 0.0, "frames": frames}
    if verbose:
        for cat in cat_iou:
            print("Category {}: IoU is {} and MAE is {}".format(cat, res["category_iou"][cat], res["category_mae"][cat]))
        print("The Average over the dataset: IoU is {} and MAE is {}".format(res["dataset_iou"], res["dataset_mae"]))
        print("The Average over sequences IoU is {}".format(res["sequence_iou"]))
        print("Success: Processed {} frames".format(frames))
    if davis_metrics:
        per, tot = _davis_summary(cat_j, cat_f, skip_ends)
        res["category_f"] = {k: float(np.mean(v)) for k, v in cat_f.items()}
        res["category_davis"], res["davis"] = per, tot
        if verbose:
            _print_davis_table(per, tot)
    return res


def evaluate_ensemble(learner, n_steps=None, save_dir=None, verbose=True):
    """The loop of test_generator_ensemble.py:_test_masks (:20-125) over learner.inference() of the augmented graph:
    per frame the IoU / MAE of every central crop are averaged; with `save_dir` the per-frame buffers the offline
    post-processing reads are written as result_<k>.mat with the reference's keys (img_1_%03d, pred_mask_%03d,
    gt_mask_%03d, :101-111).  Like the reference, the first frame of a category enters its list with the LAST crop's
    score instead of the crop mean (:70-75)."""
    import os
    cat_iou, cat_mae = {}, {}
    crops = learner.test_crops
    if n_steps is None:
        n_steps = int(learner.test_samples)
    frames = 0
    for _ in range(n_steps):
        try:
            inf = learner.inference(None)
        except StopIteration:
            if verbose:
                print("End of testing dataset")
            break
        outs, fname = inf["outs"], inf["img_fname"]
        c_iou, c_mae = [], []
        iou = mae = 0.0
        for crop in crops:
            gt, pm = outs["gt_masks"][crop], outs["pred_masks"][crop]
            if gt is None:  # synthetic data: no annotation
                gt = outs["gt_masks"][crop] = np.zeros_like(np.asarray(pm), dtype=np.float32)
            res = compute_IoU(gt_mask=gt, pred_mask_f=pm)
            if isinstance(res, tuple):
                iou, out_mask = res
            else:  # both empty: the reference returns a bare 1 (and would fail to unpack it); score it as 1 / all-background
                iou, out_mask = 1.0, np.zeros_like(np.asarray(pm), dtype=bool)
            outs["pred_masks"][crop] = out_mask
            mae = compute_mae(gt_mask=gt, pred_mask_f=out_mask)
            c_iou.append(iou)
            c_mae.append(mae)
        name = fname.decode("utf-8") if isinstance(fname, (bytes, bytearray)) else str(fname)
        parts = name.split("/")
        category = parts[-2] if len(parts) > 1 else "all"
        if category in cat_iou:
            cat_iou[category].append(float(np.mean(c_iou)))
            cat_mae[category].append(float(np.mean(c_mae)))
        else:
            cat_iou[category], cat_mae[category] = [float(iou)], [float(mae)]
        if save_dir:
            import scipy.io as sio
            d = os.path.join(save_dir, category)
            os.makedirs(d, exist_ok=True)
            mat = {}
            for crop in crops:
                k = int(crop * 100)
                mat["img_1_{:03d}".format(k)] = outs["img_1s"][crop]
                mat["pred_mask_{:03d}".format(k)] = outs["pred_masks"][crop]
                mat["gt_mask_{:03d}".format(k)] = outs["gt_masks"][crop]
            sio.savemat(os.path.join(d, "result_{}.mat".format(len(cat_iou[category]))), mat)
        frames += 1
    tot_iou = sum(sum(v) for v in cat_iou.values())
    tot_mae = sum(sum(v) for v in cat_mae.values())
    res = {"category_iou": {k: float(np.mean(v)) for k, v in cat_iou.items()},
           "category_mae": {k: float(np.mean(v)) for k, v in cat_mae.items()},
           "dataset_iou": tot_iou / max(frames, 1), "dataset_mae": tot_mae / max(frames, 1), "frames": frames}
    if verbose:
        for cat in cat_iou:
            print("Category {}: IoU is {} and MAE is {}".format(cat, res["category_iou"][cat], res["category_mae"][cat]))
        print("The Average over the dataset: IoU is {} and MAE is {}".format(res["dataset_iou"], res["dataset_mae"]))
        print("Success: Processed {} frames".format(frames))
    return res
