"""CPU: the host side of the DAVIS-2016 measures (evaluation.f_from_counts / davis_statistics / boundary_radius) and the argument
parsing of the davis_eval subcommand.  The device side is tests/test_davis_metrics_gpu.py."""
import numpy as np
import pytest


def test_f_from_counts_cases():
    from unsupervised_detection_amd.evaluation import f_from_counts
    # (n_fg, n_gt, fg_match, gt_match) -> (F, precision, recall)
    cases = [((0, 7, 0, 0), (0.0, 1.0, 0.0)),       # empty prediction boundary: precision 1, recall 0
             ((5, 0, 0, 0), (0.0, 0.0, 1.0)),       # empty ground-truth boundary: precision 0, recall 1
             ((0, 0, 0, 0), (1.0, 1.0, 1.0)),       # both empty
             ((100, 100, 66, 66), (2 * 0.66 * 0.66 / (0.66 + 0.66), 0.66, 0.66)),
             ((10, 40, 5, 10), (2 * 0.5 * 0.25 / 0.75, 0.5, 0.25)),
             ((10, 40, 0, 0), (0.0, 0.0, 0.0))]     # p + r == 0
    for c, (f, p, r) in cases:
        got = f_from_counts(np.array(c, dtype=np.int64))
        assert (float(got[0]), float(got[1]), float(got[2])) == (f, p, r), c
    f, p, r = f_from_counts(np.array([c for c, _ in cases], dtype=np.int64))
    assert f.shape == (6,) and f.dtype == np.float64
    assert f.tolist() == [w[0] for _, w in cases] and p.tolist() == [w[1] for _, w in cases] and r.tolist() == [w[2] for _, w in cases]


def test_davis_statistics_values():
    from unsupervised_detection_amd.evaluation import davis_statistics
    v = np.linspace(0.9, 0.3, 10)
    s = davis_statistics(v, skip_ends=False)
    assert set(s) == {"mean", "recall", "decay"}
    # bins: ids = round(linspace(1, 10, 5) + 1e-10) - 1 = [0, 2, 5, 7, 9]; first v[0:3], last v[7:10]
    assert abs(s["mean"] - 0.6) < 1e-12 and s["recall"] == 0.6 and abs(s["decay"] - (v[0:3].mean() - v[7:10].mean())) < 1e-12
    assert abs(s["decay"] - 0.4666666666666667) < 1e-12
    assert davis_statistics(v, skip_ends=True) == davis_statistics(v[1:-1], skip_ends=False)
    assert davis_statistics(v) == davis_statistics(v, skip_ends=True)  # the DAVIS-2016 protocol is the default
    assert davis_statistics(list(v), skip_ends=False) == s


def test_davis_statistics_short_lists_and_nan():
    from unsupervised_detection_amd.evaluation import davis_statistics
    for n in range(0, 6):
        for skip in (False, True):
            s = davis_statistics(np.full(n, 0.75), skip_ends=skip)
            if n - 2 * skip >= 1:
                assert s == {"mean": 0.75, "recall": 1.0, "decay": 0.0}, (n, skip)
            else:
                assert all(np.isnan(x) for x in s.values()), (n, skip)
    # NaN frames are ignored by the means
    v = np.array([0.8, np.nan, 0.6, 0.4, np.nan, 0.2])
    s = davis_statistics(v, skip_ends=False)
    assert abs(s["mean"] - 0.5) < 1e-12
    # ids = round(linspace(1, 6, 5) + 1e-10) - 1 = [0, 1, 3, 4, 5]: first bin v[0:2] = (0.8, nan), last v[4:6] = (nan, 0.2)
    assert abs(s["decay"] - 0.6) < 1e-12
    assert s["recall"] == 2 / 6  # mean(v > 0.5), the formula: a NaN frame is not recalled
    assert all(np.isnan(x) for x in (davis_statistics([np.nan, np.nan], skip_ends=False)[k] for k in ("mean", "decay")))


def test_boundary_radius_rule():
    from unsupervised_detection_amd.evaluation import BOUND_TH, boundary_radius
    assert BOUND_TH == 0.008
    assert boundary_radius(192, 384) == 4 and boundary_radius(480, 854) == 8 and boundary_radius(2160, 3840) == 36
    assert boundary_radius(480, 854, 0.008) == 8
    assert boundary_radius(480, 854, 3) == 3 and boundary_radius(10, 10, 1) == 1
    assert boundary_radius(30, 40, 0.1) == 5  # exactly 5.0: no rounding up past an integer


def test_davis_eval_arguments():
    from unsupervised_detection_amd.cli import parse_davis_eval_args
    a = parse_davis_eval_args(["--results_dir", "/x"])
    assert (a.results_dir, a.mask_key, a.threshold, a.bound_th, a.keep_ends) == ("/x", "pred_mask", 0.5, 0.008, False)
    a = parse_davis_eval_args(["--results_dir", "/x", "--mask_key", "soft_mask", "--threshold", "0.3", "--bound_th", "5", "--keep_ends"])
    assert (a.mask_key, a.threshold, a.bound_th, a.keep_ends) == ("soft_mask", 0.3, 5.0, True)
    for bad in ([], ["--results_dir", "/x", "--mask_key", "flow"]):
        with pytest.raises(SystemExit):
            parse_davis_eval_args(bad)


def test_davis_metrics_flag_is_off_by_default():
    from unsupervised_detection_amd.config import default_flags, parse_flags
    assert default_flags().davis_metrics is False and parse_flags([]).davis_metrics is False
    assert parse_flags(["--davis_metrics"]).davis_metrics is True
