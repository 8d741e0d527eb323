"""CPU: motion-compensated linking (native_motion.flow_displacements, native_tracks.link_detections(disp=...), csrc/motion.hip and the
motion form of csrc/tracks.hip) -- the numpy restatements of the two definitions, the hand-built translating blobs, what
the random inputs of the GPU comparison promise, the C entry points' argument checks, the wrappers' host validation, the parameters and
flags, the records' clamp, restore_results_dir(tracks={"motion": ...}) on numpy stand-ins and the header's sentences.

displacements_np restates include/udet.h's float32 arithmetic operation by operation; links_motion_np is test_tracks.links_np with the
predecessor's rank image gathered through the displacements first, bridge_motion_np test_track_gaps.bridge_np on that stage 1.
tests/test_motion_link_gpu.py compares the kernels with them for exact equality."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import test_track_gaps
from test_components import DENSITIES, _tree_files, ragged_masks
from test_detections import detect_np, select_labels_np
from test_native_results import SEQS
from test_track_gaps import GAP_FIELDS, bridge_np, sequence_inputs
from test_tracks import LINK_OK, LINK_ORDER, TracksNp, _np, greedy_match, hand_cases, inputs_np, links_np, moving_sequence, rank_map, rects, run_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 70), (67, 1), (9, 13), (33, 65), (130, 259)]
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ restatement ----
def pack_np(dx, dy):
    """dx in the low 16 bits, dy in the high 16, both signed -> int32."""
    dx, dy = np.asarray(dx, np.int64), np.asarray(dy, np.int64)
    return ((dx & 0xffff) | ((dy & 0xffff) << 16)).astype(np.uint32).view(np.int32)


def unpack_np(disp):
    d = np.asarray(disp, np.int32).astype(np.int64)
    return ((d & 0xffff) ^ 0x8000) - 0x8000, d >> 16


def displacements_np(flow, H, W):
    """include/udet.h, udet_flow_displacements_ragged, for one sample: flow [fh, fw, 2] float32 -> packed int32 [H, W].  Every line is one
    float32 operation on float32 operands, so every operation is rounded once."""
    flow = np.asarray(flow, F32)
    fh, fw = flow.shape[:2]

    def taps(size, cells):
        ratio = F32(cells) / F32(size)
        g = np.arange(size, dtype=F32) + F32(0.5)
        g = g * ratio
        g = g - F32(0.5)
        g = np.minimum(np.maximum(g, F32(0)), F32(cells - 1))
        lo = np.floor(g).astype(np.int64)
        return lo, np.minimum(lo + 1, cells - 1), g - lo.astype(F32)
    x0, x1, ax = taps(W, fw)
    y0, y1, ay = taps(H, fh)
    ax, ay = ax[None, :, None], ay[:, None, None]
    with np.errstate(all="ignore"):
        f00, f01, f10, f11 = flow[y0][:, x0], flow[y0][:, x1], flow[y1][:, x0], flow[y1][:, x1]

        def lerp(p, q, a):
            d = q - p
            d = a * d
            return p + d
        val = lerp(lerp(f00, f01, ax), lerp(f10, f11, ax), ay)
        assert val.dtype == F32 and ax.dtype == F32
        r = np.rint(val * np.array([F32(W) / F32(fw), F32(H) / F32(fh)], F32))
        r = np.clip(np.where(np.isnan(r), F32(0), r), -32768, 32767).astype(np.int64)
    return pack_np(r[..., 0], r[..., 1])


def gather_np(image, disp, fill=-1):
    """image [H, W] read at (x + dx, y + dy); `fill` where that lies outside the frame."""
    image = np.asarray(image)
    H, W = image.shape
    dx, dy = unpack_np(np.asarray(disp).reshape(H, W))
    y, x = np.mgrid[0:H, 0:W]
    xs, ys = x + dx, y + dy
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    out = np.full((H, W), fill, np.int64)
    out[inside] = image[ys[inside], xs[inside]]
    return out


def links_motion_np(labels_list, dets, counts, link, min_iou_permille, disp_list, carry=None):
    """include/udet.h, udet_link_detections_motion_ragged: links_np with one change -- the predecessor's ranks are gathered through the
    frame's displacements (disp_list: per frame the packed [H, W] int32) before the pairs are counted; disp of a frame that is not linked
    is not looked at."""
    dets, counts = _np(dets).astype(np.int64), _np(counts).astype(np.int64)
    n, k = dets.shape[:2]
    out = SimpleNamespace(inter=np.zeros((n, k, k), np.int64), match=np.full((n, k), -1, np.int32), ids=np.full((n, k), -1, np.int32),
                          linked=np.zeros(n, np.int32), seq_tracks=np.zeros(n, np.int32), next_id=0)
    rows = [min(max(int(c[2]), 0), k) for c in counts]
    prev = None
    if carry is not None:
        prev = (_np(carry.labels).reshape(carry.hw), _np(carry.dets).astype(np.int64), min(max(int(_np(carry.counts)[2]), 0), k),
                _np(carry.ids).reshape(-1))
        out.next_id = int(_np(carry.next_id).reshape(-1)[0])
    for i in range(n):
        lab = np.asarray(labels_list[i])
        if not (int(link[i]) != 0 and prev is not None and prev[0].shape == lab.shape):
            if i:
                out.seq_tracks[i - 1] = out.next_id
            out.ids[i, :rows[i]] = np.arange(rows[i])
            out.next_id = rows[i]
        else:
            out.linked[i] = 1
            ra = gather_np(rank_map(prev[0], prev[1], prev[2]).reshape(lab.shape), disp_list[i]).ravel()
            rb = rank_map(lab, dets[i], rows[i]).ravel()
            both = (ra >= 0) & (rb >= 0)
            out.inter[i] = np.bincount(ra[both] * k + rb[both], minlength=k * k).reshape(k, k)
            match = greedy_match(out.inter[i], prev[1][:prev[2], 1], dets[i, :rows[i], 1], min_iou_permille)
            for b in range(rows[i]):
                if b in match:
                    out.match[i, b], out.ids[i, b] = match[b], prev[3][match[b]]
                else:
                    out.ids[i, b] = out.next_id
                    out.next_id += 1
        prev = (lab, dets[i], rows[i], out.ids[i])
    out.seq_tracks[n - 1] = out.next_id
    return out


def bridge_motion_np(labels_list, dets, counts, link, permille, max_gap, disp_list, history=None):
    """include/udet.h, udet_link_detections_gap_motion_ragged: bridge_np with links_motion_np as its stage 1 (gap_inter stays co-located).
    bridge_np looks its stage 1 up by name, so the name is lent to the motion link for the call."""
    plain = test_track_gaps.links_np
    test_track_gaps.links_np = lambda l, d, c, ln, pm, carry=None: links_motion_np(l, d, c, ln, pm, disp_list, carry)
    try:
        return bridge_np(labels_list, dets, counts, link, permille, max_gap, history)
    finally:
        test_track_gaps.links_np = plain


# ---------------------------------------------------------------------------------------------------------------- inputs ----
def sequences(density):
    """The six sequences of tests/test_tracks_gpu.py: one per size, cut from the largest random frame of that density, and their flags."""
    base = ragged_masks(density)[5]
    frames, link = [], []
    for j, (h, w) in enumerate(SIZES):
        seq = moving_sequence(base[:h, :w], 3 + j % 2, 10 + j)
        frames += seq
        link += [0] + [1] * (len(seq) - 1)
    return frames, link


def smooth_fields(shapes, seed, grid=(3, 4), reach=3.0):
    """Per frame a smooth displacement field: a random flow of up to `reach` pixels on a coarse grid given at the frame's own scale (so
    the scale factors are those of the header), through displacements_np.  Returns (flows [n, gh, gw, 2], per-frame packed disp)."""
    rng = np.random.default_rng(seed)
    gh, gw = grid
    flows = np.empty((len(shapes), gh, gw, 2), F32)
    for i, (H, W) in enumerate(shapes):
        flows[i] = rng.uniform(-reach, reach, (gh, gw, 2)).astype(F32) * np.array([gw / W, gh / H], F32)
    return flows, [displacements_np(flows[i], H, W) for i, (H, W) in enumerate(shapes)]


def random_fields(shapes, seed):
    """Per frame a per-pixel random field whose sources leave the frame on every side, with the extremes of the 16-bit range in it."""
    rng = np.random.default_rng(seed)
    out = []
    for H, W in shapes:
        dx, dy = rng.integers(-W - 2, W + 3, (H, W)), rng.integers(-H - 2, H + 3, (H, W))
        flat = H * W
        for j, v in enumerate((32767, -32768, -32767)):
            dx.reshape(-1)[(7 * j) % flat], dy.reshape(-1)[(11 * j + 3) % flat] = v, v
        out.append(pack_np(dx, dy))
    return out


def onto_root(hw, root):
    """A field that maps every pixel of an H x W frame onto the pixel `root` (row-major) of the frame before it."""
    H, W = hw
    y, x = np.mgrid[0:H, 0:W]
    return pack_np(int(root) % W - x, int(root) // W - y)


BLOB_STEPS = ((9, -6), (-8, 7), (11, 0))    # (dx, dy) per frame
BLOB_STARTS = ((0, 27), (54, -4), (0, 9))  # (x, y) of the 5 x 5 blobs in frame 0; the first two leave the 33 x 65 frame in part


def translating_blobs(n=6, hw=(33, 65)):
    """Three 5 x 5 blobs that move further than their extent per frame -> (frames, per-frame exact disp, per-frame blob boxes).  The
    displacement of frame c is constant over each blob's pixels: minus its step, so that the source is where the blob was."""
    H, W = hw
    frames, disps, boxes = [], [], []
    for t in range(n):
        m, dx, dy, bx = np.zeros(hw, np.uint8), np.zeros(hw, np.int64), np.zeros(hw, np.int64), []
        for (sx, sy), (x0, y0) in zip(BLOB_STEPS, BLOB_STARTS):
            x, y = x0 + t * sx, y0 + t * sy
            ya, yb, xa, xb = max(y, 0), min(y + 5, H), max(x, 0), min(x + 5, W)
            m[ya:yb, xa:xb] = 1
            dx[ya:yb, xa:xb], dy[ya:yb, xa:xb] = -sx, -sy
            bx.append((ya, xa, yb, xb))
        frames.append(m)
        disps.append(pack_np(dx, dy))
        boxes.append(bx)
    return frames, disps, boxes


# Per frame, in rank order (the larger area first, then the smaller root), with the blobs A, B, C in the order of BLOB_STARTS.  Frame 0:
# C (row 9), A (row 27), B (5 pixels) -> C = 0, A = 1, B = 2.  Frame 1: B (row 3), C (row 9), A (row 21).  Frame 2: C (row 9), B (row 10),
# A (row 15).  Frames 3 and 4: A (row 9, column 27; row 3), C, B.  Frame 5: C (25 pixels), A (10 pixels, row 0), B (10 pixels, row 31).
BLOB_IDS = [[0, 1, 2], [2, 0, 1], [0, 2, 1], [1, 0, 2], [1, 0, 2], [0, 1, 2]]


# ----------------------------------------------------------------------------------------------------------------- tests ----
def test_pack_and_displacements_restated():
    dx, dy = np.array([0, 1, -1, 32767, -32768, 5]), np.array([0, -1, 1, -32768, 32767, -7])
    p = pack_np(dx, dy)
    assert p.dtype == np.int32 and p[1] == np.int32(-65536 + 1) and p[2] == 0x1ffff
    assert all(np.array_equal(a, b) for a, b in zip(unpack_np(p), (dx, dy)))
    # a grid of the sample's own size: the centres coincide, every ratio is 1 and disp = rint(flow), ties to even
    H, W = 5, 7
    flow = np.zeros((H, W, 2), F32)
    flow[..., 0] = np.arange(W, dtype=F32)[None, :] - 2.5   # -2.5 .. 3.5: ties on every column
    flow[..., 1] = (np.arange(H, dtype=F32)[:, None] - 2) * 1.5
    dx, dy = unpack_np(displacements_np(flow, H, W))
    assert dx[0].tolist() == [-2, -2, 0, 0, 2, 2, 4] and dy[:, 0].tolist() == [-3, -2, 0, 2, 3]
    # a constant flow stays constant and is scaled to native pixels; 1 x 1 grids and samples
    dx, dy = unpack_np(displacements_np(np.full((2, 3, 2), 2.0, F32), 9, 13))
    assert (dx == round(2 * 13 / 3)).all() and (dy == 9).all()
    assert unpack_np(displacements_np(np.array([[[3.0, -4.0]]], F32), 1, 1)) == (3, -4)
    # a NaN gives 0 -- and so does an infinity, whose difference with itself is one; values beyond the range are clamped
    got = [unpack_np(displacements_np(np.array([[uv]], F32), 2, 3)) for uv in ((np.nan, np.inf), (-np.inf, 1e9), (-1e9, 40000.0), (32767.4, -32768.6))]
    assert [(int(dx[1, 2]), int(dy[1, 2])) for dx, dy in got] == [(0, 0), (0, 32767), (-32768, 32767), (32767, -32768)]
    assert all((dx == dx[0, 0]).all() and (dy == dy[0, 0]).all() for dx, dy in got)


def test_zero_displacement_is_the_co_located_link():
    for name, (frames, k, permille) in hand_cases().items():
        labels, dets, counts = inputs_np(frames, k)
        want = links_np(labels, dets, counts, [1] * len(frames), permille)
        got = links_motion_np(labels, dets, counts, [1] * len(frames), permille, [np.zeros(f.shape, np.int32) for f in frames])
        assert all(np.array_equal(getattr(got, f), getattr(want, f)) for f in ("inter", "match", "ids", "linked", "seq_tracks")), name
        assert got.next_id == want.next_id
    _, labels, dets, counts = sequence_inputs(3, 0.3, 64, 8)
    zero = [np.zeros(np.asarray(l).shape, np.int32) for l in labels]
    got, want = bridge_motion_np(labels, dets, counts, [1] * 7, 100, 3, zero), bridge_np(labels, dets, counts, [1] * 7, 100, 3)
    assert all(np.array_equal(getattr(got, f), getattr(want, f)) for f in GAP_FIELDS) and got.next_id == want.next_id
    assert test_track_gaps.links_np is links_np  # the name went back


def test_translating_blobs_keep_their_ids():
    frames, disps, boxes = translating_blobs()
    for t in range(5):  # further than their extent: no blob shares a pixel with any blob of the next frame
        assert not (frames[t] & frames[t + 1]).any()
    labels, dets, counts = inputs_np(frames, 4)
    assert counts[:, 2].tolist() == [3] * 6
    plain = links_np(labels, dets, counts, [1] * 6, 100)
    assert plain.next_id == 18 and not plain.inter.any()
    got = links_motion_np(labels, dets, counts, [1] * 6, 100, disps)
    assert got.next_id == 3 and got.seq_tracks.tolist() == [0] * 5 + [3] and (got.match[1:, :3] >= 0).all()
    assert got.ids[:, :3].tolist() == BLOB_IDS
    # the ids follow the blobs: a row's box says which blob it is, and that blob's id is its rank in frame 0
    first = {boxes[0][j]: int(np.flatnonzero([tuple(r[2:6]) == boxes[0][j] for r in dets[0, :3]])[0]) for j in range(3)}
    for t in range(6):
        for b in range(3):
            j = [bx for bx in boxes[t]].index(tuple(int(v) for v in dets[t, b, 2:6]))
            assert got.ids[t, b] == first[boxes[0][j]], (t, b)
    # every iou is 1 while the blob is inside the frame in both frames; entering or leaving it, the visible part is what is shared
    from unsupervised_detection_amd.native_tracks import track_records
    from test_detections import DetectionsNp
    trk = TracksNp(got, labels, DetectionsNp(dets, counts), None)
    trk.motion = True
    recs = track_records([[{} for _ in range(3)] for _ in range(6)], trk)
    whole = 0
    for t in range(1, 6):
        for b, r in enumerate(recs[t]):
            a = int(got.match[t, b])
            small, large = sorted((int(dets[t - 1, a, 1]), int(dets[t, b, 1])))
            assert got.inter[t, a, b] == small  # every pixel of the smaller of the two (the blob in part outside the frame) is shared
            assert r["iou"] == small / large
            whole += small == large == 25
    assert whole >= 8


@pytest.mark.parametrize("density", DENSITIES)
def test_the_random_fields_change_the_overlap(density):
    """What keeps the GPU comparison from being vacuous: with the smooth fields the restatement's inter differs from the co-located one
    on at least half of the linked frames, and both link something."""
    frames, link = sequences(density)
    labels, dets, counts = inputs_np(frames, 16)
    _, disps = smooth_fields([f.shape for f in frames], 21)
    plain, moved = links_np(labels, dets, counts, link, 100), links_motion_np(labels, dets, counts, link, 100, disps)
    linked = np.flatnonzero(plain.linked)
    assert plain.linked.tolist() == link == moved.linked.tolist()
    differ = sum(not np.array_equal(plain.inter[i], moved.inter[i]) for i in linked)
    assert 2 * differ >= len(linked), (differ, len(linked))
    assert (moved.match >= 0).sum() > 10 and moved.inter.sum() > 0
    # sources outside the frame on every side, and a field that maps a whole frame onto one pixel: inter exceeds the predecessor's area
    wild = links_motion_np(labels, dets, counts, link, 100, random_fields([f.shape for f in frames], 5))
    assert not np.array_equal(wild.inter, plain.inter)
    a = int(counts[-2, 2]) - 1  # onto the root of the predecessor's smallest row
    onto = [np.zeros(f.shape, np.int32) for f in frames[:-1]] + [onto_root(frames[-1].shape, dets[-2, a, 0])]
    one = links_motion_np(labels, dets, counts, link, 1, onto)
    rows = int(counts[-1, 2])
    assert a >= 1 and one.inter[-1, a, :rows].tolist() == dets[-1, :rows, 1].tolist() and int(one.inter[-1].sum()) == int(dets[-1, :rows, 1].sum())
    assert one.inter[-1, a, 0] > dets[-2, a, 1] and one.match[-1, 0] == a  # inter > area_a, and the union area_a + area_b - inter is still positive


def test_gap_form_restated_only_stage_one_is_warped():
    for size_index, density, k, conn in ((3, 0.3, 64, 8), (5, 0.45, 16, 4)):
        _, labels, dets, counts = sequence_inputs(size_index, density, k, conn)
        _, disps = smooth_fields([np.asarray(l).shape for l in labels], 3)
        for g in (1, 3):
            moved, plain = bridge_motion_np(labels, dets, counts, [1] * 7, 100, g, disps), bridge_np(labels, dets, counts, [1] * 7, 100, g)
            s1 = links_motion_np(labels, dets, counts, [1] * 7, 100, disps)
            assert all(np.array_equal(getattr(moved, f), getattr(s1, f)) for f in ("inter", "match", "linked"))
            assert np.array_equal(moved.gap_inter, plain.gap_inter) and not np.array_equal(moved.inter, plain.inter)
            assert (moved.back >= 2).sum() > 0


# ------------------------------------------------------------------------------------------------ arguments and the header ----
DISP_OK = dict(flow=64, n=2, fh=8, fw=16, offsets=64, hw=64, max_h=30, max_w=53, total=3180, disp=64, stream=None)
DISP_ORDER = "flow n fh fw offsets hw max_h max_w total disp stream".split()
DISP_BAD = ([dict(**{p: None}) for p in ("flow", "offsets", "hw", "disp")] +
            [dict(n=0), dict(n=65536), dict(fh=0), dict(fw=0), dict(fh=32768), dict(fw=32768), dict(max_h=0), dict(max_w=0), dict(total=0),
             dict(flow=68), dict(disp=66)])
MOTION_ORDER = LINK_ORDER[:LINK_ORDER.index("ws")] + ["disp"] + LINK_ORDER[LINK_ORDER.index("ws"):]
GAP_OK = dict(labels=64, n=2, offsets=64, hw=64, max_h=30, max_w=53, total=3180, dets=256, counts=512, k=16, link=64, max_gap=2, m=0, h_labels=None,
              h_h=0, h_w=0, h_dets=None, h_counts=None, h_ids=None, h_open=None, h_next=None, permille=100, inter=1024, match=64, ids=128,
              linked=192, seq=320, next_id=448, gap_inter=2048, back=64, prev=128, open=192, disp=64, ws=64, ws_bytes=1 << 20, stream=None)
GAP_ORDER = ("labels n offsets hw max_h max_w total dets counts k link max_gap m h_labels h_h h_w h_dets h_counts h_ids h_open h_next permille "
             "inter match ids linked seq next_id gap_inter back prev open disp ws ws_bytes stream").split()


def test_library_exports_and_refuses_bad_arguments():
    """UDET_ERR_ARG (-5) with udet_last_error() set, before anything is enqueued: runs without a GPU (the pointers are never read)."""
    from unsupervised_detection_amd._ffi import lib
    for change in DISP_BAD:
        a = dict(DISP_OK, **change)
        assert lib.udet_flow_displacements_ragged(*[a[p] for p in DISP_ORDER]) == -5 and b"flow_displacements_ragged" in lib.udet_last_error(), change
    ok = dict(LINK_OK, disp=64)
    for change in (dict(disp=None), dict(disp=66), dict(labels=None), dict(n=0), dict(k=65), dict(permille=0), dict(ws=None), dict(ws_bytes=64),
                   dict(c_h=30, c_w=53)):
        a = dict(ok, **change)
        assert lib.udet_link_detections_motion_ragged(*[a[p] for p in MOTION_ORDER]) == -5, change
        assert b"link_detections_motion_ragged" in lib.udet_last_error(), change
    for change in (dict(disp=None), dict(disp=66), dict(labels=None), dict(max_gap=0), dict(max_gap=9), dict(gap_inter=None), dict(m=1),
                   dict(ws_bytes=64)):
        a = dict(GAP_OK, **change)
        assert lib.udet_link_detections_gap_motion_ragged(*[a[p] for p in GAP_ORDER]) == -5, change
        assert b"link_detections_gap_motion_ragged" in lib.udet_last_error(), change
    # the co-located entries keep their names in their messages
    assert lib.udet_link_detections_ragged(*[dict(LINK_OK, k=0)[p] for p in LINK_ORDER]) == -5
    assert lib.udet_last_error().startswith(b"link_detections_ragged:")


def test_the_header_says_what_the_symbols_do():
    hdr = open(os.path.join(ROOT, "include", "udet.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    assert re.search(r"\bint udet_flow_displacements_ragged\(const float\* flow, int n, int fh, int fw, const long long\* offsets,", hdr)
    assert re.search(r"\bint udet_link_detections_motion_ragged\(const int\* labels, int n,", hdr)
    assert re.search(r"\bint udet_link_detections_gap_motion_ragged\(const int\* labels, int n,", hdr)
    for sentence in ("dx in the low 16 bits, dy in the high 16, both signed", "every operation rounded once and nothing fused",
                     "gx = ((float)x + 0.5f) * rx - 0.5f, clamped to [0, fw - 1]", "x0 = (int)floorf(gx), x1 = min(x0 + 1, fw - 1), ax = gx - (float)x0",
                     "top = f00 + ax * (f01 - f00), bot = f10 + ax * (f11 - f10), val = top + ay * (bot - top)",
                     "dx = rint(u * sx) and dy = rint(v * sy), ties to even; a NaN gives 0; the result is clamped to -32768 .. 32767",
                     "no LDS, no atomics, no workspace", "fh or fw outside 1..32767",
                     "labels_p(x + dx, y + dy) = root_a + 1", "A position whose source lies outside the frame contributes nothing",
                     "disp of a frame that is not linked is not read", "inter may exceed area_a", "In the gap entry only stage 1 is warped",
                     "gap_inter at distances d >= 2 stays co-located", "Every index a kernel forms is bounded whatever disp holds"):
        assert sentence in flat, sentence
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "7.12" in design and "udet_flow_displacements_ragged" in design and "udet_link_detections_gap_motion_ragged" in design
    assert "Chaining displacements" in design or "chained displacements" in design.lower()


def test_wrappers_validate_before_the_device_is_touched():
    import torch
    from unsupervised_detection_amd.native_motion import BackwardFlow, check_flow_arguments, flow_displacements, motion_params, motion_size
    from unsupervised_detection_amd.native_results import Detections, Tracks, link_detections, track_params
    from unsupervised_detection_amd.ragged import PackedLayout
    hw = [(30, 53), (30, 53)]
    total, k = 2 * 30 * 53, 4
    layout = PackedLayout.packed(hw)
    flow = torch.zeros((2, 8, 16, 2))  # host tensors: anything that got past the validation would fail on them, not launch
    assert check_flow_arguments(flow, layout) == (layout, 8, 16) and check_flow_arguments(flow, SimpleNamespace(layout=layout))[0] is layout
    for match, f, l in (("float32", flow.double(), layout), ("4-D", flow[0], layout), ("one field per frame", flow[:1], layout),
                        ("one field per frame", torch.zeros((2, 8, 16, 3)), layout), ("1..32767", torch.zeros((2, 0, 16, 2)), layout),
                        ("PackedLayout", flow, [0, 1590]), ("float32", flow.numpy(), layout), ("CUDA", flow, layout)):
        with pytest.raises(ValueError, match=match):
            flow_displacements(f, l)
    lab = torch.zeros(total, dtype=torch.int32)
    det = Detections(torch.zeros((2, k, 9), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.int64), layout, 1, k)
    for match, disp in (("disp", torch.zeros(total)), ("disp", torch.zeros(total - 1, dtype=torch.int32)), ("disp", [0] * total),
                        ("disp", torch.zeros((2, total // 2), dtype=torch.int32)), ("CUDA", torch.zeros(total, dtype=torch.int32))):
        for gap in (0, 2):
            with pytest.raises(ValueError, match=match):
                link_detections(lab, det, disp=disp, max_gap=gap)
    # the parameters
    assert motion_size((64, 128)) == (64, 128) and motion_params(None) == motion_params({}) == {"size": (384, 640)}
    assert motion_params({"size": [128, 64]}) == {"size": (128, 64)}
    for bad in ((0, 64), (64, 100), (64,), 64, (64.0, 64), (True, 64), (-64, 64), (64, 32768 + 64)):
        with pytest.raises(ValueError, match="motion size"):
            motion_size(bad)
    with pytest.raises(ValueError, match="motion"):
        motion_params({"sise": (64, 64)})
    assert track_params({"motion": None}) == track_params({}) == {"min_iou": 0.1}
    assert track_params({"motion": {}}) == {"min_iou": 0.1, "motion": {"size": (384, 640)}}
    assert track_params({"min_iou": 0.3, "max_gap": 2, "motion": {"size": (64, 128)}}) == {"min_iou": 0.3, "max_gap": 2, "motion": {"size": (64, 128)}}
    assert list(track_params({"motion": {}, "max_gap": 1})) == ["min_iou", "max_gap", "motion"]
    for bad in ({"motion": 1}, {"motion": {"size": (65, 64)}}, {"motion": {"size": None, "x": 1}}):
        with pytest.raises(ValueError, match="tracks"):
            track_params(bad)
    # the provider checks its own arguments and builds no network before it is called
    p = BackwardFlow(size=(64, 128), flow_batch=2)
    assert p.size == (64, 128) and p.flow_fn is None and p.prev is None
    p.prev = 1
    p.reset()
    assert p.prev is None
    for kw in (dict(size=(64, 100)), dict(flow_batch=0), dict(flow_batch=True)):
        with pytest.raises(ValueError):
            BackwardFlow(**kw)
    # a Tracks records how it was linked
    parts = [torch.zeros(s, dtype=d) for s, d in (((2, k, k), torch.int64), ((2, k), torch.int32), ((2, k), torch.int32), (2, torch.int32),
                                                  (2, torch.int32), (1, torch.int32))]
    assert Tracks(*parts, lab, det).motion is False and Tracks(*parts, lab, det, motion=True).motion is True


def test_the_iou_of_the_records_is_clamped_under_motion_only():
    from test_detections import DetectionsNp
    from unsupervised_detection_amd.native_results import detection_records, track_records
    frames = [rects((8, 18), (1, 1, 3, 3)), rects((8, 18), (1, 1, 5, 9))]  # 4 pixels, then 32
    labels, dets, counts = inputs_np(frames, 2)
    y, x = np.mgrid[0:8, 0:18]
    onto = [np.zeros((8, 18), np.int32), pack_np(1 - x, 1 - y)]  # every pixel of frame 1 came from (1, 1)
    r = links_motion_np(labels, dets, counts, [1, 1], 100, onto)
    assert r.inter[1, 0, 0] == 32 and dets[0, 0, 1] == 4 and r.match[1, 0] == 0  # inter > area_a, union = 4
    det = DetectionsNp(dets, counts)
    recs = detection_records(det, [255] * 2)
    trk = TracksNp(r, labels, det, None)
    assert track_records(recs, trk)[1][0]["iou"] == 8.0  # not linked with motion: what it reports today
    trk.motion = True
    got = track_records(recs, trk)
    assert got[1][0]["iou"] == 1.0 and got[1][0]["track"] == 0 and got[0][0]["iou"] is None
    plain = links_np(labels, dets, counts, [1, 1], 100)
    trk = TracksNp(plain, labels, det, None)
    trk.motion = True
    assert track_records(recs, trk)[1][0]["iou"] == 4 / 32  # below 1: untouched


# ------------------------------------------------------------------------------------------------------ restore_results_dir ----
class FramesNp(object):
    """Stand-in for the loaded frames: only their paths (the stand-in provider needs no pixels)."""

    def __init__(self, paths):
        self.paths = list(paths)


class FlowNp(object):
    """Stand-in for BackwardFlow: a seeded constant flow per frame of up to two pixels, at the asked size; notes its calls."""

    def __init__(self, size, calls):
        self.size, self.calls, self.seen = size, calls, 0

    def reset(self):
        self.calls.append("reset")
        self.seen = 0

    def __call__(self, frames):
        n = len(frames.paths)
        self.calls.append(n)
        out = np.empty((n,) + tuple(self.size) + (2,), F32)
        for i in range(n):
            rng = np.random.default_rng(100 + self.seen + i)
            out[i] = rng.integers(-2, 3, 2).astype(F32)  # (u, v): whole native pixels once scaled back
        self.seen += n
        return out


def displace_np(flow, labelled):
    """Stand-in for flow_displacements over the stand-ins: displacements_np per frame.  The stand-in flow is given in native pixels, so it
    is brought to grid pixels first (the kernel's scale factors bring it back)."""
    out = []
    for i, lab in enumerate(labelled.labels):
        H, W = np.asarray(lab).shape
        fh, fw = flow[i].shape[:2]
        out.append(displacements_np(flow[i] * np.array([fw / W, fh / H], F32), H, W))
    return out


def link_motion_np(calls):
    """Stand-in for link_detections with disp: links_motion_np (bridge_motion_np with max_gap) on the labels select_labels_np kept."""
    from test_track_gaps import history_np

    class GapTracksNp(TracksNp):
        def __init__(self, r, labels, det, carry, max_gap):
            TracksNp.__init__(self, r, labels, det, carry)
            self.max_gap, self.motion = max_gap, True

        def host_gaps(self):
            return self.r.gap_inter, self.r.back, self.r.prev, self.r.open

        def tail(self):
            if not self.max_gap:
                return TracksNp.tail(self)
            return history_np(self.r, self.labels, self.detections.dets, self.detections.counts, self.max_gap, self.carry)

    def link(labelled, det, link=None, carry=None, min_iou=0.1, max_gap=0, disp=None):
        from unsupervised_detection_amd.native_results import min_iou_permille
        calls.append((list(link), carry is not None, min_iou, max_gap, disp is not None))
        if max_gap:
            r = bridge_motion_np(labelled.labels, det.dets, det.counts, link, min_iou_permille(min_iou), max_gap, disp, carry)
        else:
            r = links_motion_np(labelled.labels, det.dets, det.counts, link, min_iou_permille(min_iou), disp, carry)
        return GapTracksNp(r, labelled.labels, det, carry, max_gap)
    return link


@pytest.mark.parametrize("gap", [0, 1])
def test_restore_results_dir_with_motion(tmp_path, gap):
    det = dict(select=select_labels_np([]), detect=detect_np, detections={"min_area": 2, "max_detections": 3}, load_images=FramesNp,
               displace=displace_np)
    tracks = dict({"min_iou": 0.2, "motion": {"size": (64, 128)}}, **({"max_gap": gap} if gap else {}))
    calls3, calls7, flows3, flows7 = [], [], [], []
    out3, js3, _ = run_tree(tmp_path, "m3", True, 3, tracks=tracks, link=link_motion_np(calls3), motion_flow=FlowNp((64, 128), flows3), **det)
    out7, js7, _ = run_tree(tmp_path, "m7", True, 7, tracks=tracks, link=link_motion_np(calls7), motion_flow=FlowNp((64, 128), flows7), **det)
    assert calls3 == [([0, 1, 1], False, 0.2, gap, True), ([1, 1, 1], True, 0.2, gap, True), ([1], True, 0.2, gap, True)] * 2
    assert calls7 == [([0] + [1] * 6, False, 0.2, gap, True)] * 2
    assert flows3 == ["reset", 3, 3, 1] * 2 and flows7 == ["reset", 7] * 2
    assert js3 == js7 and js3["tracks"] == dict({"min_iou": 0.2}, **({"max_gap": gap} if gap else {}))
    assert js3["track_motion"] == {"size": [64, 128]} and list(js3)[-1] == "track_motion"
    f3, f7 = _tree_files(out3), _tree_files(out7)
    assert sorted(f3) == sorted(f7) and all(f3[k] == f7[k] for k in f3)  # batch 3 and batch 7: the same files, byte for byte
    with open(os.path.join(out3, "native_eval.json")) as f:
        assert json.load(f) == json.loads(json.dumps(js3))
    # the same tree without motion: only native_eval.json and the linked files may differ, and the schema is what it was
    from test_track_gaps import link_gap_np
    plain_link = link_gap_np([]) if gap else __import__("test_tracks").link_np([])
    plain = {k: v for k, v in tracks.items() if k != "motion"}
    out0, js0, _ = run_tree(tmp_path, "m0", True, 3, tracks=plain, link=plain_link, **{k: v for k, v in det.items() if k not in ("load_images", "displace")})
    f0 = _tree_files(out0)
    assert sorted(f0) == sorted(f3) and "track_motion" not in js0 and {k: v for k, v in js3.items() if k not in ("track_motion", "sequences")} == \
        {k: v for k, v in js0.items() if k != "sequences"}
    linked = {"native_eval.json"} | {os.path.join(d, s + ".json") for d in ("detections", "tracks") for s in SEQS}
    assert all(f0[k] == f3[k] for k in f0 if k not in linked)
    assert any(f0[k] != f3[k] for k in linked if k != "native_eval.json")  # the flow moved something
    for seq in SEQS:
        with open(os.path.join(out3, "detections", seq + ".json")) as f:
            got = json.load(f)
        with open(os.path.join(out0, "detections", seq + ".json")) as f:
            was = json.load(f)
        assert list(got) == list(was) and all([set(d) for d in got[s]] == [set(d) for d in was[s]] for s in got)
        assert all(d["iou"] is None or 0 < d["iou"] <= 1.0 for s in got for d in got[s])


def test_motion_absent_or_none_changes_nothing(tmp_path):
    """tracks without "motion", or with "motion": None: neither callable runs, link receives no disp= and every file equals a run
    without the key."""
    from test_tracks import link_np

    def never(*a, **k):
        raise AssertionError("called without motion")
    det = dict(select=select_labels_np([]), detect=detect_np, detections={"min_area": 2, "max_detections": 3})
    a, b, c = [], [], []
    out0, js0, _ = run_tree(tmp_path, "a", True, 3, tracks={"min_iou": 0.2}, link=link_np(a), **det)
    out1, js1, _ = run_tree(tmp_path, "b", True, 3, tracks={"min_iou": 0.2, "motion": None}, link=link_np(b), motion_flow=never, displace=never,
                            load_images=never, **det)
    out2, js2, _ = run_tree(tmp_path, "c", True, 3, tracks={"min_iou": 0.2}, link=link_np(c), motion_flow=never, displace=never, load_images=never, **det)
    assert a == b == c and js0 == js1 == js2 and "track_motion" not in js0 and js0["tracks"] == {"min_iou": 0.2}
    f0, f1, f2 = _tree_files(out0), _tree_files(out1), _tree_files(out2)
    assert sorted(f0) == sorted(f1) == sorted(f2) and all(f0[k] == f1[k] == f2[k] for k in f0)
    with pytest.raises(ValueError, match="tracks"):
        run_tree(tmp_path, "d", True, 3, tracks={"motion": {"size": (60, 64)}}, link=never, **det)


def test_cli_flags():
    from unsupervised_detection_amd import cli
    from unsupervised_detection_amd.config import default_flags, parse_flags
    base = ["--results_dir", "D", "--out_dir", "O", "--root_dir", "R"]
    a = cli.parse_restore_results_args(base + ["--detections", "--tracks"])
    assert a.track_motion is False and tuple(a.track_motion_size) == (384, 640) and cli._tracks(a) == {"min_iou": 0.1}
    a = cli.parse_restore_results_args(base + ["--detections", "--tracks", "--track_motion"])
    assert cli._tracks(a) == {"min_iou": 0.1, "motion": {"size": (384, 640)}}
    a = cli.parse_restore_results_args(base + ["--detections", "--tracks", "--track_max_gap", "2", "--track_motion", "--track_motion_size", "64", "128"])
    assert cli._tracks(a) == {"min_iou": 0.1, "max_gap": 2, "motion": {"size": (64, 128)}}
    for bad, said in ((["--track_motion"], "it needs --tracks"), (["--detections", "--track_motion"], "it needs --tracks"),
                      (["--track_motion_size", "64", "128"], "it needs --tracks"),
                      (["--detections", "--tracks", "--track_motion_size", "64", "128"], "it needs --track_motion"),
                      (["--detections", "--tracks", "--track_motion", "--track_motion_size", "64", "100"], "multiples of 64"),
                      (["--detections", "--tracks", "--track_motion", "--track_motion_size", "0", "64"], "multiples of 64"),
                      (["--detections", "--tracks", "--track_motion", "--track_motion_size", "-64", "64"], "multiples of 64")):
        with pytest.raises(SystemExit) as e:
            cli.parse_restore_results_args(base + bad)
        assert said in str(e.value), bad
    d = default_flags()
    assert d.track_motion is False and tuple(d.track_motion_size) == (384, 640) and cli._tracks(d) is None
    native = ["--native_resolution", "--generate_visualization", "--test_save_dir", "D"]
    f = parse_flags(native + ["--detections", "--tracks", "--track_motion", "--track_motion_size", "128", "192"])
    cli.check_native_flags(f)
    assert cli._tracks(f) == {"min_iou": 0.1, "motion": {"size": (128, 192)}}
    assert cli._tracks(parse_flags(native + ["--detections", "--tracks"])) == {"min_iou": 0.1}
    with pytest.raises(SystemExit) as e:
        cli.check_native_flags(parse_flags(native + ["--detections", "--track_motion"]))
    assert "it needs --tracks" in str(e.value)
    pp = ["--buffer_dir", "B", "--out_dir", "O", "--benchmark", "--root_dir", "R"]
    assert cli._tracks(cli.parse_post_process_args(pp + ["--detections", "--tracks", "--track_motion"])) == {"min_iou": 0.1, "motion": {"size": (384, 640)}}
    with pytest.raises(SystemExit) as e:
        cli.parse_post_process_args(pp + ["--detections", "--track_motion"])
    assert "it needs --tracks" in str(e.value)
    for flag in ("--track_motion", "--track_motion_size"):
        assert flag in cli.__doc__
