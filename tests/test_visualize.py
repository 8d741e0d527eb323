"""CPU: the visualisation / summary layer that needs no device -- exported symbols, the histogram bucket limits, the SummaryWriter
file layout, the --summary_dir flag, and the fixture tests/golden/visualize.npz (the reference's own flow_to_image outputs, written by
tools/make_visualize_golden.py) against a numpy restatement of the precision mix the kernel implements."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "visualize.npz")


def color_wheel():
    """make_color_wheel restated: six ramps, one channel full, one rising / falling as floor(255 i / len)."""
    rows = []
    for s, (n, full, ramp) in enumerate(((15, 0, 1), (6, 1, 0), (4, 1, 2), (11, 2, 1), (13, 2, 0), (6, 0, 2))):
        for i in range(n):
            r = np.floor(255 * i / n)
            row = [0.0, 0.0, 0.0]
            row[full] = 255.0
            row[ramp] = 255.0 - r if s & 1 else r
            rows.append(row)
    return np.asarray(rows, np.float64)


def flow_to_image_np(flow):
    """flow_to_image + compute_color with the reference's arithmetic on a float32 flow under numpy 2: the running maximum radius is
    float32, everything from the division by (maxrad + eps) on is float64."""
    f = np.array(flow, np.float32)
    n, h, w, _ = f.shape
    wheel = color_wheel()
    out = np.zeros((n, h, w, 3), np.uint8)
    maxrad = np.float32(-1)
    for i in range(n):
        u, v = f[i, :, :, 0], f[i, :, :, 1]
        unknown = (np.abs(u) > 1e7) | (np.abs(v) > 1e7)
        u[unknown] = 0
        v[unknown] = 0
        rad32 = np.sqrt(u * u + v * v)
        assert rad32.dtype == np.float32
        maxrad = max(maxrad, np.max(rad32))
        den = np.float64(maxrad) + np.finfo(np.float64).eps
        ud, vd = u.astype(np.float64) / den, v.astype(np.float64) / den
        rad = np.sqrt(ud * ud + vd * vd)
        fk = (np.arctan2(-vd, -ud) / np.pi + 1) / 2 * 54 + 1
        k0 = np.floor(fk).astype(int)
        k1 = k0 + 1
        k1[k1 == 56] = 1
        fr = fk - k0
        for c in range(3):
            col = (1 - fr) * (wheel[k0 - 1, c] / 255) + fr * (wheel[k1 - 1, c] / 255)
            col = np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
            out[i, :, :, c] = np.floor(255 * col)
    return out


def test_symbols_are_exported():
    from unsupervised_detection_amd import _ffi
    for n in ("udet_flow_to_image", "udet_flow_to_image_workspace_bytes", "udet_overlay_mask", "udet_grad_histogram",
              "udet_grad_histogram_workspace_bytes", "udet_histogram_limits"):
        assert hasattr(_ffi.lib, n), n
    assert _ffi.lib.udet_flow_to_image_workspace_bytes(3) >= 3 * 4
    assert _ffi.lib.udet_grad_histogram_workspace_bytes(5) >= 1551 * 8


def test_bucket_limits_are_tensorflows_defaults():
    from unsupervised_detection_amd.visualize import bucket_limits
    lim = bucket_limits()
    assert lim.shape == (1551,) and lim.dtype == np.float64
    assert np.all(np.diff(lim) > 0)
    assert lim[775] == 0 and lim[776] == 1e-12 and lim[-1] == np.finfo(np.float64).max
    assert np.array_equal(lim, -lim[::-1])
    # the generating loop itself, in Python's double arithmetic
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    assert len(pos) == 774 and np.array_equal(lim[776:1550], np.asarray(pos))


def test_summary_writer_layout(tmp_path):
    from PIL import Image
    from unsupervised_detection_amd.visualize import SummaryWriter
    d = tmp_path / "sum"
    wr = SummaryWriter(str(d))
    keys = ("generator", "recover", "red_rate", "red_rate_compl", "reconstruction_loss", "reconstruction_compl_loss",
            "denominator_red_rate", "denominator_red_rate_compl")
    for step in (4, 8):
        wr.add_scalars(step, {k: 0.5 * step + i for i, k in enumerate(keys)})
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    wr.add_image(4, "PWC_Flow", img)
    names = ["a/kernel", "a/bias"]
    stats = np.arange(10, dtype=np.float64).reshape(2, 5)
    counts = np.zeros((2, 1551), np.uint32)
    counts[1, 775] = 3
    wr.add_histograms(4, "generator", names, stats, counts)
    lines = [json.loads(l) for l in (d / "scalars.jsonl").read_text().splitlines()]
    assert [l["step"] for l in lines] == [4, 8] and set(lines[0]) == {"step", *keys} and lines[1]["recover"] == 5.0
    with Image.open(d / "images" / "step_00000004_PWC_Flow.png") as im:
        assert im.size == (7, 5) and np.array_equal(np.asarray(im), img)
    z = np.load(d / "histograms" / "step_00000004_generator.npz")
    assert list(z["names"]) == names and np.array_equal(z["stats"], stats) and np.array_equal(z["counts"], counts)
    assert z["limits"].shape == (1551,)


def test_summary_dir_flag():
    from unsupervised_detection_amd.config import default_flags, parse_flags
    assert parse_flags([]).summary_dir == "" and default_flags().summary_dir == ""
    assert parse_flags(["--summary_dir", "/tmp/x"]).summary_dir == "/tmp/x"


def test_host_postprocessing_keeps_rgb():
    from unsupervised_detection_amd.models.utils.general_utils import postprocess_image, postprocess_mask
    from unsupervised_detection_amd.models.utils import flow_utils
    assert callable(flow_utils.flow_to_image)
    img = np.array([[[-0.5, 0.0, 0.5]]], np.float32)
    assert postprocess_image(img).tolist() == [[[0, 127, 255]]]
    m = postprocess_mask(np.array([[[1.0], [0.0]]]))
    assert m.dtype == np.uint8 and m.tolist() == [[[0, 255, 0], [0, 0, 0]]]


def test_fixture_equals_the_mixed_precision_restatement():
    """Guards the fixture against regeneration under another numpy: the float32-max / float64-colour restatement above equals the
    reference's own images exactly, the wheel included; and the two 8 x 8 fields are on either side of the `* 0.75` branch."""
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert np.array_equal(z["wheel"], color_wheel())
    for name, shape in (("a", (3, 12, 20, 2)), ("b", (3, 33, 47, 2)), ("hi", (1, 8, 8, 2)), ("lo", (1, 8, 8, 2))):
        flow, img = z["flow_" + name], z["img_" + name]
        assert flow.shape == shape and flow.dtype == np.float32 and img.dtype == np.uint8
        assert np.isfinite(flow).all() and np.abs(flow).max() < 1e7
        assert np.array_equal(flow_to_image_np(flow), img), name
    # sample 1 of flow_a is normalised by sample 0's maximum: on its own it would look different
    assert not np.array_equal(flow_to_image_np(z["flow_a"][1:2])[0], z["img_a"][1])
    for name, beyond in (("hi", True), ("lo", False)):
        f = z["flow_" + name][0]
        rad = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1])
        y, x = np.unravel_index(np.argmax(rad), rad.shape)
        den = np.float64(rad.max()) + np.finfo(np.float64).eps
        r = np.sqrt((f[y, x, 0] / den) ** 2 + (f[y, x, 1] / den) ** 2)
        assert (r > 1) == beyond, (name, r)
