"""CPU: unsupervised_detection_amd/pil_tables.py -- the coefficient blocks and the pass validation shared by the restore tables
(native_results) and the soft-score tables (post_processing), and the two table builders pinned byte for byte to what they produced
before they shared them."""
import hashlib

import numpy as np
import pytest

from test_native_results import SIZES

# sha256(tab.tobytes() + coef.tobytes()) of build_restore_tables / sha256(geom.tobytes() + coef.tobytes()) of soft_score_geometry,
# computed at commit 72e5904 ("Report every connected component as a scored box at native size"), the last one with a builder of its own
# in each module
RESTORE_DIGESTS = [
    ((SIZES, 12, 24, 0.9), "2639158e60e84748c3140e675a2ed5550bc4dc523f45ecb70ff0b7721ec8cf1b"),
    (([(480, 854)], 192, 384, 0.9), "ecca2c4508781c9c33e617e3a6e6c02902ce5cbc6af8af6e6972cb030571071b"),
    (([(12, 24)], 12, 24, 1.0), "b886c6fedd58419f0013b06be220f31c8420416019dbecc1eb5e86ed8f876a10")]
SOFT_DIGESTS = [
    ((2, (85, 90, 95, 100), 90.0, (192, 384)), "37dc806ae729702c814625e2fc645999dc08a1cbf8a03bb3596e4afc2b6c7b13"),
    ((2, (85, 90, 95, 100), 90.0, (24, 40)), "03c413fcc283f9d8680e3f8c169128fc927c3a76f504af74fb44771e46ab3a0f"),
    ((2, (85, 90, 95, 100), 90.0, (70, 131)), "2db1087924094eee9ac47b4fc01c63f6aa4ef037dd91f089e51936165b19c509"),
    ((1, (85, 100), 90.0, (24, 40)), "1d31598890ef39b24e3e14359f86a34d9087c9622ec9aaf174b2a5738bbec9db"),
    ((3, (90,), 90.0, (24, 40)), "a6d5aad1fef49027346447c8ebb5570a8035d949d59be1da1cea8bbb52a16976")]


@pytest.mark.parametrize("args, digest", RESTORE_DIGESTS)
def test_restore_tables_are_the_parents(args, digest):
    from unsupervised_detection_amd.native_results import build_restore_tables
    _, tab, coef = build_restore_tables(*args)
    assert tab.dtype == np.int32 and coef.dtype == np.int32
    assert hashlib.sha256(tab.tobytes() + coef.tobytes()).hexdigest() == digest


@pytest.mark.parametrize("args, digest", SOFT_DIGESTS)
def test_soft_score_tables_are_the_parents(args, digest):
    from unsupervised_detection_amd.post_processing import soft_score_geometry
    geom, coef = soft_score_geometry(*args)
    assert geom.dtype == np.int32 and coef.dtype == np.int32
    assert hashlib.sha256(geom.tobytes() + coef.tobytes()).hexdigest() == digest


def test_block_builder():
    from unsupervised_detection_amd.pil_tables import CoefBlocks, pil_coeffs_host
    blocks = CoefBlocks()
    empty = blocks.coef()
    assert empty.dtype == np.int32 and len(empty) == 1  # never empty: the calls take no NULL table
    assert blocks.block(24, 24) == (-1, -1, 0) and len(blocks.coef()) == 1
    first = blocks.block(24, 47)
    kk, bounds, ks = pil_coeffs_host(24, 47)
    assert first == (0, 47 * ks, ks)
    size = len(blocks.coef())
    assert size == kk.size + bounds.size
    second = blocks.block(12, 8)
    assert second[0] == size and second[1] == size + 8 * second[2]
    grown = blocks.coef()
    assert blocks.block(24, 47) == first and blocks.block(12, 8) == second  # a repeated (in, out): the same offsets ...
    assert np.array_equal(blocks.coef(), grown)                             # ... and nothing added
    assert grown.dtype == np.int32 and grown.flags["C_CONTIGUOUS"]
    assert np.array_equal(grown[:kk.size].reshape(47, ks), kk) and np.array_equal(grown[kk.size:size].reshape(47, 2), bounds)


def test_check_pass_refusals():
    """Each refusal once, on a block the builder made, broken in one integer."""
    from unsupervised_detection_amd.pil_tables import CoefBlocks, check_pass
    blocks = CoefBlocks()
    k, b, ks = blocks.block(24, 47)
    blocks.block(12, 8)  # something behind the block under test: an index past it still lies inside coef
    coef = blocks.coef()
    check_pass(coef, (k, b, ks), 24, 47, "sample 0", "horizontal")
    check_pass(coef, (-1, -1, 0), 24, 24, "sample 0", "horizontal")

    def refused(match, block=(k, b, ks), n_in=24, n_out=47, at=None, value=None):
        c = coef.copy()
        if at is not None:
            c[at] = value
        with pytest.raises(ValueError, match="row 7: .*" + match):
            check_pass(c, block, n_in, n_out, "row 7", "vertical")
    refused("vertical coefficient index", block=(-1, b, ks))  # kk and bounds go together
    refused("vertical coefficient index", block=(k, -1, ks))
    refused("vertical pass 24 -> 47 cannot be skipped", block=(-1, -1, 0))
    refused("vertical coefficient index", block=(k, b, 0))
    refused("vertical coefficient index", block=(len(coef) - 47 * ks + 1, b, ks))  # the kk block ends one past coef
    refused("vertical coefficient index", block=(k, len(coef) - 2 * 47 + 1, ks))   # the bounds block ends one past coef
    refused("tap of the vertical pass", at=b, value=-1)                  # a first tap before the input
    refused("tap of the vertical pass", at=b + 1, value=0)               # no tap at all
    refused("tap of the vertical pass", at=b + 1, value=ks + 1)          # more taps than the coefficient row holds
    refused("tap of the vertical pass", at=b + 2 * 46, value=24)         # the last output's only tap lies past the input
    assert coef[b + 2 * 19:b + 2 * 22].tolist() == [9, 2, 9, 2, 10, 2]
    refused("vertical pass move backwards", at=b + 2 * 20, value=8)      # a first tap before its predecessor's
    refused("vertical pass move backwards", at=b + 2 * 20 + 1, value=1)  # a window that ends before its predecessor's
