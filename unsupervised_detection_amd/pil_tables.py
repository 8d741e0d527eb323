"""Host tables of Pillow's 8-bit BILINEAR resampler (numpy only) for the batched kernels of csrc/pil_resample.h: the coefficients of one
pass (pil_coeffs_host), the concatenated coefficient blocks the kernels index (CoefBlocks) and their validation (check_pass) -- the only
bounds check those kernels have.  native_results.build_restore_tables / check_restore_tables and post_processing.soft_score_geometry /
check_soft_score_tables are geometry plus calls into this module."""
import functools
import math

import numpy as np

@functools.lru_cache(maxsize=None)
def pil_coeffs_host(in_size, out_size):
    """Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter (host side, exactly Pillow's double
    arithmetic): int32 arrays kk [out][ksize] and bounds [out][2] = (first tap, taps), and ksize.  Cached per (in, out): the arrays
    are shared, not to be written to."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [0.0] * ksize
        ww = 0.0
        for x in range(xmax):
            v = abs((x + xmin - center + 0.5) * ss)
            w[x] = 1.0 - v if v < 1.0 else 0.0
            ww += w[x]
        for x in range(ksize):
            v = w[x] / ww if (x < xmax and ww != 0.0) else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[xx] = (xmin, xmax)
    return kk, bounds, ksize


class CoefBlocks(object):
    """The coefficient buffer of one table set: one block (kk [out][ks], then bounds [out][2]) per distinct (in, out) length."""

    def __init__(self):
        self._chunks, self._where, self._pos = [], {}, 0

    def block(self, n_in, n_out):
        """(kk offset, bounds offset, ksize) of the pass n_in -> n_out inside coef(); (-1, -1, 0) for equal lengths: the pass is skipped."""
        key = (int(n_in), int(n_out))
        if key[0] == key[1]:
            return -1, -1, 0
        if key not in self._where:
            kk, bounds, ks = pil_coeffs_host(*key)
            self._where[key] = (self._pos, self._pos + kk.size, ks)
            self._chunks.extend([kk.reshape(-1), bounds.reshape(-1)])
            self._pos += kk.size + bounds.size
        return self._where[key]

    def coef(self):
        """The concatenated blocks, contiguous int32; never empty (the calls take no NULL table)."""
        return np.ascontiguousarray(np.concatenate(self._chunks), dtype=np.int32) if self._chunks else np.zeros(1, np.int32)


def check_pass(coef, block, n_in, n_out, where, name):
    """ValueError, opening with `where` and naming the pass (`name`: "horizontal" / "vertical"), unless the kernels may follow
    block = (k, b, ks) for a pass n_in -> n_out: both offsets negative only for n_in == n_out; otherwise the kk block [n_out][ks] at k
    and the bounds block [n_out][2] at b inside coef, every tap inside the input and inside its coefficient row, first taps and ends
    non-decreasing (as Pillow's are: a tile's source rows are those between its first row's first tap and its last row's end)."""
    k, b, ks = (int(v) for v in block)
    n_in, n_out = int(n_in), int(n_out)
    if (k < 0) != (b < 0):
        raise ValueError("{}: the {} coefficient index leaves coef (kk and bounds go together)".format(where, name))
    if k < 0:
        if n_in != n_out:
            raise ValueError("{}: the {} pass {} -> {} cannot be skipped".format(where, name, n_in, n_out))
        return
    if ks < 1 or k + n_out * ks > len(coef) or b + 2 * n_out > len(coef):
        raise ValueError("{}: the {} coefficient index leaves coef".format(where, name))
    lo, cnt = np.asarray(coef[b:b + 2 * n_out], dtype=np.int64).reshape(-1, 2).T
    if (lo < 0).any() or (cnt < 1).any() or (cnt > ks).any() or (lo + cnt > n_in).any():
        raise ValueError("{}: a tap of the {} pass leaves its input of {} or its coefficient row of {}".format(where, name, n_in, ks))
    if (np.diff(lo) < 0).any() or (np.diff(lo + cnt) < 0).any():
        raise ValueError("{}: the tap windows of the {} pass move backwards".format(where, name))
