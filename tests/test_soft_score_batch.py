"""CPU: the host side of the batched soft score -- soft_score_geometry's integers and coefficient blocks, the table check,
the exports and argument errors of udet_post_soft_score_batch, the --score_batch flag and the unchanged default of buffer_to_soft_score.
Also the inputs tests/test_soft_score_batch_gpu.py shares."""
import ctypes
import inspect
import os

import numpy as np
import pytest

CROPS = (85, 90, 95, 100)
# geometry row columns (post_processing.SOFT_SCORE_GEOM = 16)
MODE, SY0, SX0, SH, SW, HH, WW, Y0, X0, HK, HB, HKS, VK, VB, VKS = range(15)


def blob_mask(h, w, seed):
    """tests/test_post_processing.py::_mask with the blob kept clear of the border: the border mean stays at or below 0.05 whatever the
    size (the noise's 0.05 bounds it once the Gaussian has died out at the border)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0.45, 0.55) * (h - 1), rng.uniform(0.45, 0.55) * (w - 1)
    m = np.exp(-(((yy - cy) / (0.12 * h)) ** 2 + ((xx - cx) / (0.1 * w)) ** 2)) + 0.05 * rng.random((h, w))
    return (m / m.max()).astype(np.float32)


def border_mean(s):
    """oracle_post.sanity_check's expression (float64)."""
    s = s.astype(np.float64)
    H, W = s.shape
    return (s[0:2].sum() + s[H - 2:].sum() + s[:, 0:2].sum() + s[:, W - 2:].sum()) / (4.0 * W + 4.0 * H)


def ensemble(n, ns, nc, h, w, seed, edges=(), const=()):
    """[n, 2, ns, nc, h, w] float32 blob masks; edges: (frame, direction, shift index, crop index) slots that hold an all-ones mask (border
    mean 1); const: slots constant at 0.25 (border mean 0.25, cscale == 0).  Every border mean is at least 0.1 away from 0.6."""
    out = np.empty((n, 2, ns, nc, h, w), np.float32)
    for k in range(n * 2 * ns * nc):
        out.reshape(-1, h, w)[k] = blob_mask(h, w, seed * 1000 + k)
    for e in edges:
        out[e] = 1.0
    for c in const:
        out[c] = 0.25
    for m in out.reshape(-1, h, w):
        assert abs(border_mean(m) - 0.6) >= 0.1
    return out


# ------------------------------------------------------------------------------------------------------------ geometry ----
@pytest.mark.parametrize("hw, down85, up95, up100", [
    ((17, 23), (16, 21, 0, 1), (16, 21, 0, 1), (15, 20, 1, 1)),
    ((24, 40), (22, 37, 1, 1), (22, 37, 1, 1), (21, 36, 1, 2)),
    ((70, 131), (66, 123, 2, 4), (66, 124, 2, 3), (62, 117, 4, 7)),
    ((192, 384), (181, 362, 5, 11), (181, 363, 5, 10), (172, 345, 10, 19))])
def test_geometry_integers(hw, down85, up95, up100):
    from unsupervised_detection_amd import post_processing as PP
    H, W = hw
    geom, coef = PP.soft_score_geometry(2, CROPS, 90.0, hw)
    assert geom.dtype == np.int32 and coef.dtype == np.int32 and geom.shape == (8, PP.SOFT_SCORE_GEOM) and coef.ndim == 1
    for si in (0, 1):
        d, u95, u100 = geom[si * 4 + 0], geom[si * 4 + 2], geom[si * 4 + 3]
        # crop 85: the whole mask shrunk to hh x ww and placed at (y0, x0)
        assert d[MODE] == 1 and tuple(d[[SY0, SX0, SH, SW]]) == (0, 0, H, W) and tuple(d[[HH, WW, Y0, X0]]) == down85
        # crops 95 / 100: the window hh x ww at (y0, x0) of the mask enlarged to the whole canvas
        for row, want in ((u95, up95), (u100, up100)):
            assert row[MODE] == 1 and tuple(row[[SH, SW, SY0, SX0]]) == want and tuple(row[[HH, WW, Y0, X0]]) == (H, W, 0, 0)
    # shift 1 / crop 90: the identity; shift 2 / crop 90: a rectify whose two passes are both skipped
    assert geom[1][MODE] == 0
    r = geom[5]
    assert r[MODE] == 1 and tuple(r[[SY0, SX0, SH, SW, HH, WW, Y0, X0]]) == (0, 0, H, W, H, W, 0, 0) and r[HK] < 0 and r[VK] < 0
    PP.check_soft_score_tables(geom, coef, hw)


def test_down_and_up_widths_differ_at_70x131():
    from unsupervised_detection_amd import post_processing as PP
    geom, _ = PP.soft_score_geometry(1, CROPS, 90.0, (70, 131))
    assert geom[0][WW] == 123 and geom[2][SW] == 124


def test_coefficient_blocks_equal_pil_coeffs_host():
    from unsupervised_detection_amd import post_processing as PP
    H, W = 70, 131
    geom, coef = PP.soft_score_geometry(2, CROPS, 90.0, (H, W))
    seen = 0
    for row in geom:
        if row[MODE] == 0:
            continue
        for (k, b, ks), n_in, n_out in (((row[HK], row[HB], row[HKS]), row[SW], row[WW]), ((row[VK], row[VB], row[VKS]), row[SH], row[HH])):
            if n_in == n_out:
                assert k < 0
                continue
            kk, bounds, ksize = PP._pil_coeffs_host(int(n_in), int(n_out))
            assert ks == ksize and k >= 0 and b >= 0
            assert np.array_equal(coef[k:k + n_out * ks].reshape(n_out, ks), kk)
            assert np.array_equal(coef[b:b + 2 * n_out].reshape(n_out, 2), bounds)
            seen += 1
    assert seen == 12  # three resampled crops x two shifts x two passes
    # the two shifts share their blocks: one pair per distinct (in, out)
    assert np.array_equal(geom[0][HK:], geom[4][HK:])
    sizes = {(W, 123), (H, 66), (124, W), (66, H), (117, W), (62, H)}
    assert len(coef) == sum(PP._pil_coeffs_host(i, o)[0].size + 2 * o for i, o in sizes)


def test_other_ensemble_sizes():
    from unsupervised_detection_amd import post_processing as PP
    geom, _ = PP.soft_score_geometry(1, (85, 100), 90.0, (24, 40))
    assert geom[:, MODE].tolist() == [1, 1]  # no identity row
    geom, coef = PP.soft_score_geometry(3, (90,), 90.0, (24, 40))
    assert geom[:, MODE].tolist() == [0, 1, 1] and (geom[1:, HK] < 0).all() and (geom[1:, VK] < 0).all() and len(coef) >= 1
    with pytest.raises(ValueError):
        PP.soft_score_geometry(0, CROPS, 90.0, (24, 40))
    with pytest.raises(ValueError, match="row 0"):
        PP.soft_score_geometry(1, (1,), 90.0, (24, 40))  # int(24 / 90) = 0 rows


def test_table_check_rejects_and_names_the_row():
    from unsupervised_detection_amd import post_processing as PP
    hw = (24, 40)
    geom, coef = PP.soft_score_geometry(2, CROPS, 90.0, hw)
    g, c = PP.check_soft_score_tables(geom, coef, hw)
    assert g.dtype == np.int32 and c.dtype == np.int32 and np.array_equal(g, geom) and np.array_equal(c, coef)

    def broken(row, col, value):
        g = geom.copy()
        g[row, col] = value
        return g
    with pytest.raises(ValueError, match="row 0.*patch.*canvas"):
        PP.check_soft_score_tables(broken(0, Y0, 3), coef, hw)  # 22 rows at y0 = 3 end past row 24
    with pytest.raises(ValueError, match="row 4.*patch.*canvas"):
        PP.check_soft_score_tables(broken(4, X0, -1), coef, hw)
    with pytest.raises(ValueError, match="row 2.*window.*frame"):
        PP.check_soft_score_tables(broken(2, SX0, 4), coef, hw)
    with pytest.raises(ValueError, match="row 3.*horizontal.*coef"):
        PP.check_soft_score_tables(broken(3, HK, len(coef) - 1), coef, hw)
    with pytest.raises(ValueError, match="row 5.*vertical.*skipped"):
        PP.check_soft_score_tables(broken(5, HH, 23), coef, hw)
    with pytest.raises(ValueError, match="row 1.*mode"):
        PP.check_soft_score_tables(broken(1, MODE, 2), coef, hw)
    bad = coef.copy()
    bad[geom[0][VB] + 2 * (geom[0][HH] - 1)] = 24  # the last output row's first tap: past the mask
    with pytest.raises(ValueError, match="row 0.*tap.*vertical"):
        PP.check_soft_score_tables(geom, bad, hw)
    with pytest.raises(ValueError):
        PP.check_soft_score_tables(geom[:, :12], coef, hw)
    PP.check_soft_score_tables(broken(1, SH, 10 ** 6), coef, hw)  # the identity row's geometry is not read


# --------------------------------------------------------------------------------------------------------- the library ----
def test_new_exports_and_workspace():
    from unsupervised_detection_amd._ffi import lib
    for name in ("udet_post_soft_score_workspace_bytes", "udet_post_soft_score_batch"):
        assert hasattr(lib, name), name
    import unsupervised_detection_amd.post_processing as PP  # declares the argument types
    here = os.path.dirname(os.path.abspath(PP.__file__))
    for other in ("libudet_debug.so", "libudet_exp.so"):  # the debug hooks bind to libudet.so's; the experiment build has its own
        if os.path.exists(os.path.join(here, other)):
            assert hasattr(ctypes.CDLL(os.path.join(here, other)), "udet_post_soft_score_batch"), other
    with open(os.path.join(os.path.dirname(here), "include", "udet.h")) as f:
        assert "#define UDET_SOFT_SCORE_GEOM %d\n" % PP.SOFT_SCORE_GEOM in f.read()
    need = lib.udet_post_soft_score_workspace_bytes
    for ns, nc, h, w in ((2, 4, 192, 384), (2, 4, 17, 23), (1, 2, 24, 40), (3, 1, 4, 4)):
        one = need(1, ns, nc, h, w)
        assert one > 0 and need(16, ns, nc, h, w) == 16 * one and need(5, ns, nc, h, w) == 5 * one  # linear in n
        assert one >= 2 * ns * nc * h * w  # the patches
        assert one < (2 * ns * nc + 4) * h * w + 64 * 1024  # ... plus a little: no float64 canvas per mask
    for bad in ((0, 2, 4, 24, 40), (1, 0, 4, 24, 40), (1, 2, 0, 24, 40), (1, 2, 4, 0, 40), (1, 2, 4, 24, 0)):
        assert need(*bad) == 0


def test_argument_errors_without_a_device():
    """Argument errors are decided before the device is touched (-5 = UDET_ERR_ARG): they can be checked without one.  The pointers are host
    addresses that are never dereferenced."""
    from unsupervised_detection_amd._ffi import lib
    import unsupervised_detection_amd.post_processing  # noqa: F401
    ws_bytes = lib.udet_post_soft_score_workspace_bytes(1, 2, 4, 24, 40)
    buf = np.zeros(ws_bytes + 64, np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16  # 16-byte aligned, stands for every pointer
    good = dict(masks=p, n=1, ns=2, nc=4, h=24, w=40, geom=p, coef=p, san_t=0.6, pred=p, ws=p, ws_bytes=ws_bytes)
    cases = [dict(n=0), dict(ns=0), dict(nc=0), dict(h=0), dict(w=0), dict(n=-1), dict(h=3), dict(w=3), dict(masks=None), dict(geom=None),
             dict(coef=None), dict(pred=None), dict(ws=None), dict(san_t=float("nan")), dict(san_t=float("inf")),
             dict(ws_bytes=ws_bytes - 1), dict(ws=p + 8), dict(n=65535)]
    for change in cases:
        a = dict(good, **change)
        if "ws_bytes" not in change and set(change) & {"n", "ns", "nc", "h", "w"}:
            a["ws_bytes"] = max(lib.udet_post_soft_score_workspace_bytes(a["n"], a["ns"], a["nc"], a["h"], a["w"]), 1 << 20)
        assert lib.udet_post_soft_score_batch(a["masks"], a["n"], a["ns"], a["nc"], a["h"], a["w"], a["geom"], a["coef"], a["san_t"], a["pred"],
                                              a["ws"], a["ws_bytes"], None) == -5, change
        assert b"post_soft_score_batch" in lib.udet_last_error(), change


# ------------------------------------------------------------------------------------------------------ flag and driver ----
def test_score_batch_parser():
    from unsupervised_detection_amd import cli
    base = ["--buffer_dir", "B", "--out_dir", "O"]
    assert cli.parse_post_process_args(base).score_batch == 0
    assert cli.parse_post_process_args(base + ["--score_batch", "4"]).score_batch == 4
    with pytest.raises(SystemExit):
        cli.parse_post_process_args(base + ["--score_batch", "-1"])


def test_post_process_passes_score_batch(tmp_path, monkeypatch):
    import json
    from unsupervised_detection_amd import cli, post_processing as PP
    d = tmp_path / "buf" / "davis_shift_1" / "bear"
    d.mkdir(parents=True)
    for k in (1, 2):
        (d / ("result_%d.mat" % k)).write_bytes(b"")
    seen = []
    monkeypatch.setattr(PP, "buffer_to_soft_score", lambda *a, **k: seen.append(("soft", a, k)))
    monkeypatch.setattr(PP, "run_crf", lambda *a, **k: seen.append(("crf", a, k)) or np.float32(0.5))
    monkeypatch.setattr(PP, "run_crf_original_resolution", lambda *a, **k: seen.append(("orig", a, k)) or {})
    out = str(tmp_path / "out")
    assert cli.main(["post_process", "--buffer_dir", str(tmp_path / "buf"), "--out_dir", out, "--score_batch", "4"]) == 0
    assert seen[0][0] == "soft" and seen[0][2] == {"max_shift": 2, "dprefix": "davis_shift", "flow_batch": 8, "score_batch": 4}
    with open(os.path.join(out, "post_process.json")) as f:
        assert json.load(f)["score_batch"] == 4
    del seen[:]
    assert cli.main(["post_process", "--buffer_dir", str(tmp_path / "buf"), "--out_dir", out]) == 0
    assert "score_batch" not in seen[0][2]  # 0: the keyword is not passed at all
    with open(os.path.join(out, "post_process.json")) as f:
        assert "score_batch" not in json.load(f)


def test_defaults_keep_the_per_frame_path():
    from unsupervised_detection_amd import post_processing as PP
    assert inspect.signature(PP.buffer_to_soft_score).parameters["score_batch"].default is None
    sig = inspect.signature(PP.soft_score_batch).parameters
    assert list(sig) == ["preds", "crops", "base_crop", "san_t"]
    assert (sig["crops"].default, sig["base_crop"].default, sig["san_t"].default) == ((85, 90, 95, 100), 90.0, 0.6)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="score_batch"):
            PP.buffer_to_soft_score("nowhere", "nowhere", [], [], score_batch=bad)
