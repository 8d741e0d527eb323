#!/usr/bin/env python3
"""Writes tests/golden/visualize.npz: seeded float32 flow fields and what the REFERENCE's own flow_to_image makes of them.

    python tools/make_visualize_golden.py /path/to/unsupervised_detection

The reference's models/utils/flow_utils.py is imported at run time from the tree given on the command line (never copied), on
the TensorFlow stand-in of oracle/tf1_shim.py (the module imports tensorflow; flow_to_image itself is numpy).  The images depend on
numpy's type promotion (float32 radius, float64 from the division by maxrad + eps on): tests/test_visualize.py restates that mix and
fails if the fixture is ever regenerated under a numpy that promotes differently.

Contents (inputs hold no NaN and no |value| > 1e7 -- those cases have known-answer tests):
  flow_a [3,12,20,2]   per-sample scales 3.0 / 0.5 / 9.0: sample 1 is normalised by sample 0's maximum, sample 2 raises it
  flow_b [3,33,47,2]   odd sizes
  flow_hi, flow_lo [1,8,8,2]   the first seeds at which the pixel of maximum radius does / does not come out with rad > 1 after
                       the division and so takes / does not take the `* 0.75` branch (seed_hi, seed_lo)
  img_<name>           uint8 images of flow_to_image(flow_<name>)
  wheel [55,3]         make_color_wheel()"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import tf1_shim  # noqa: E402


def field(seed, shape, scales):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape).astype(np.float32)
    return f * np.asarray(scales, np.float32).reshape(-1, 1, 1, 1)


def max_pixel_beyond_one(f):
    """Does the pixel of maximum float32 radius of f [1,h,w,2] have a float64 radius > 1 after the reference's division?"""
    u, v = f[0, :, :, 0], f[0, :, :, 1]
    rad = np.sqrt(u ** 2 + v ** 2)
    i = np.unravel_index(np.argmax(rad), rad.shape)
    den = np.max(rad) + np.finfo(float).eps
    return bool(np.sqrt((u[i] / den) ** 2 + (v[i] / den) ** 2) > 1)


def main():
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    tf1_shim.install()
    spec = importlib.util.spec_from_file_location("ref_flow_utils", os.path.join(sys.argv[1], "models", "utils", "flow_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"flow_a": field(11, (3, 12, 20, 2), (3.0, 0.5, 9.0)), "flow_b": field(12, (3, 33, 47, 2), (1.0, 1.0, 1.0))}
    for name, want in (("hi", True), ("lo", False)):
        seed = next(s for s in range(100, 1000) if max_pixel_beyond_one(field(s, (1, 8, 8, 2), (1.0,))) == want)
        out["flow_" + name], out["seed_" + name] = field(seed, (1, 8, 8, 2), (1.0,)), np.int64(seed)
    for name in ("a", "b", "hi", "lo"):
        img = ref.flow_to_image(out["flow_" + name].copy())  # (the reference writes into its argument)
        assert img.dtype == np.float32 and np.array_equal(img, np.floor(img)) and img.min() >= 0 and img.max() <= 255
        out["img_" + name] = img.astype(np.uint8)
    out["wheel"] = ref.make_color_wheel()
    out["numpy_version"] = np.asarray(np.__version__)
    path = os.path.join(ROOT, "tests", "golden", "visualize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; seeds", int(out["seed_hi"]), int(out["seed_lo"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
