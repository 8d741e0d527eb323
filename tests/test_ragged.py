"""CPU: the packed layout (unsupervised_detection_amd/ragged.py) -- the one validator and the validators that are now
thin calls of it, PackedLayout, and the argument errors of require_tensor / workspace.  Nothing here touches a device."""
import numpy as np
import pytest
import torch

from unsupervised_detection_amd import data, native_results, ragged
from unsupervised_detection_amd.ragged import PackedLayout, check_packed_tables

SIZES = [(30, 53), (13, 26), (9, 70)]
AREAS = [h * w for h, w in SIZES]


def _old_names(buffer):
    """The validators that kept their names, each as f(offsets, hw, numel) -> (offsets, hw)."""
    def restore(off, hw, numel):
        hw = np.asarray(hw, np.int64).reshape(-1, 2)
        tab = np.zeros((len(hw), native_results.TAB), np.int32)
        tab[:, 2:4], tab[:, 4:6], tab[:, 6:] = hw, hw, (-1, -1, 0, -1, -1, 0)  # the whole frame, both passes skipped: 4 x 5 masks
        o, t, _ = native_results.check_restore_tables(off, tab, np.zeros(1, np.int32), numel, 4, 5)
        return o, t[:, 4:6]
    named = {"packed buffer": [native_results.check_component_tables, native_results.check_crf_tables,
                               lambda o, h, n: data.check_ragged_tables(o, h, 1, n)[:2]],
             "output buffer": [restore]}
    return named[buffer]


def test_check_packed_tables_and_the_old_names():
    off, hw = check_packed_tables([0, 12], [(3, 4), (2, 5)], 22)
    assert off.dtype == np.int64 and hw.dtype == np.int32 and off.tolist() == [0, 12] and hw.tolist() == [[3, 4], [2, 5]]
    assert off.flags.c_contiguous and hw.flags.c_contiguous
    check_packed_tables([14, 2], [(2, 5), (3, 4)], 24)  # any order, gaps allowed
    check_packed_tables([0, 36], [(3, 4), (2, 5)], 66, c=3)  # c elements per pixel
    cases = [("overlap", ([0, 11], [(3, 4), (2, 5)], 30)),
             ("overlap", ([13 * 26 - 5, 0], [(30, 53), (13, 26)], 30 * 53 + 13 * 26)),  # given in descending order
             ("outside the packed buffer", ([0, 12], [(3, 4), (2, 5)], 21)),
             ("outside the packed buffer", ([-1], [(3, 4)], 30)),
             ("outside the packed buffer", ([0, 30 * 53 + 1], [(30, 53), (13, 26)], 30 * 53 + 13 * 26)),
             ("2\\^31", ([0], [(1 << 16, 1 << 15)], 1 << 40)),
             ("at least 1x1", ([0], [(0, 4)], 30)),
             ("one \\(H, W\\) per offset", ([0, 1], [(1, 1)], 30)),
             ("one \\(H, W\\) per offset", ([], [], 30))]
    for match, args in cases:
        with pytest.raises(ValueError, match=match):
            check_packed_tables(*args)
        for old in _old_names("packed buffer"):
            if match == "overlap" and old is not native_results.check_component_tables and old is not native_results.check_crf_tables:
                old(*args)  # the input stage only reads its buffer: samples may share bytes there
                continue
            with pytest.raises(ValueError, match=match):
                old(*args)
    with pytest.raises(ValueError, match="outside the packed buffer"):
        check_packed_tables([0, 36], [(3, 4), (2, 5)], 65, c=3)
    check_packed_tables([0, 11], [(3, 4), (2, 5)], 30, overlap_ok=True)
    with pytest.raises(ValueError, match="65535"):
        check_packed_tables(np.arange(65536), np.ones((65536, 2), np.int64), 65536, max_samples=65535)
    with pytest.raises(ValueError, match="65535"):
        native_results.check_crf_tables(np.arange(65536), np.ones((65536, 2), np.int64), 65536)
    check_packed_tables(np.arange(65536), np.ones((65536, 2), np.int64), 65536)
    # valid tables: the old names return what the one validator returns
    for args in (([0, 12], [(3, 4), (2, 5)], 22), ([14, 2], [(2, 5), (3, 4)], 24)):
        want = check_packed_tables(*args)
        for old in _old_names("packed buffer"):
            got = old(*args)
            assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
    # the restore tables name their buffer
    restore = _old_names("output buffer")[0]
    got = restore([0, 20], [(4, 5), (4, 5)], 40)
    assert np.array_equal(got[0], [0, 20]) and got[1].tolist() == [[4, 5], [4, 5]]
    for match, args in (("outside the output buffer", ([0, 21], [(4, 5), (4, 5)], 40)), ("overlap", ([0, 19], [(4, 5), (4, 5)], 40)),
                        ("at least 1x1", ([0, 20], [(4, 5), (0, 5)], 40)), ("outside the output buffer", ([-1, 20], [(4, 5), (4, 5)], 40))):
        with pytest.raises(ValueError, match=match):
            check_packed_tables(*args, buffer="output buffer")
        with pytest.raises(ValueError, match=match):
            restore(*args)


def test_sequence_tables_share_the_range_rules():
    from unsupervised_detection_amd.post_processing import check_sequence_tables
    first, length = check_sequence_tables([4, 0], [3, 4], 7)
    assert first.dtype == np.int32 and first.tolist() == [4, 0] and length.tolist() == [3, 4]
    with pytest.raises(ValueError, match="overlap"):
        check_sequence_tables([3, 0], [3, 4], 7)
    with pytest.raises(ValueError, match="outside"):
        check_sequence_tables([4, 0], [4, 4], 7)


def test_packed_layout():
    lay = PackedLayout.packed(SIZES)
    assert (lay.n, lay.numel, lay.c, lay.max_h, lay.max_w, len(lay)) == (3, sum(AREAS), 1, 30, 70, 3)
    assert lay.offsets.tolist() == [0, AREAS[0], AREAS[0] + AREAS[1]] and lay.offsets.dtype == np.int64
    assert lay.hw.tolist() == [list(s) for s in SIZES] and lay.hw.dtype == np.int32
    assert np.array_equal(np.asarray(lay), lay.hw)  # a layout reads as its sizes
    buf = torch.arange(lay.numel, dtype=torch.int32)
    for i, (h, w) in enumerate(SIZES):
        v = lay.view(buf, i)
        assert v.shape == (h, w) and v.data_ptr() == buf.data_ptr() + 4 * int(lay.offsets[i])
        assert int(v[0, 0]) == int(lay.offsets[i]) and int(v[-1, -1]) == int(lay.offsets[i]) + h * w - 1
    rgb = PackedLayout.packed(SIZES, c=3)
    assert rgb.numel == 3 * lay.numel and rgb.offsets.tolist() == (3 * lay.offsets).tolist()
    assert rgb.view(torch.zeros(rgb.numel, dtype=torch.uint8), 2).shape == (9, 70, 3)
    assert rgb.same_as(lay, scale=3) and not rgb.same_as(lay) and not lay.same_as(rgb, scale=3) and lay.same_as(lay)
    assert lay.same_as(PackedLayout(lay.offsets, lay.hw, lay.numel)) and not lay.same_as(PackedLayout.packed(SIZES[::-1]))
    # a gap before every sample and a tail; the same samples given in descending offset order
    G = 64
    offs = [G, 2 * G + AREAS[0], 3 * G + AREAS[0] + AREAS[1]]
    numel = offs[-1] + AREAS[2] + G
    gap = PackedLayout(offs, SIZES, numel)
    assert gap.numel == numel and not gap.same_as(lay)
    assert not gap.same_as(PackedLayout(offs, SIZES, numel + 1))  # another buffer length is another layout
    big = torch.arange(numel, dtype=torch.int32)
    assert all(int(gap.view(big, i)[0, 0]) == offs[i] for i in range(3))
    desc = PackedLayout(offs[::-1], SIZES[::-1], numel)
    assert desc.offsets.tolist() == offs[::-1] and desc.hw.tolist() == [list(s) for s in SIZES[::-1]]
    assert all(torch.equal(desc.view(big, 2 - i), gap.view(big, i)) for i in range(3))
    assert gap.same_as(PackedLayout(3 * np.asarray(offs), SIZES, 3 * numel, 3), scale=1) is False
    assert PackedLayout(3 * np.asarray(offs), SIZES, 3 * numel, 3).same_as(gap, scale=3)
    with pytest.raises(ValueError, match="overlap"):
        PackedLayout([0, AREAS[0] - 1], SIZES[:2], numel)
    with pytest.raises(ValueError, match="outside the output buffer"):
        PackedLayout(offs, SIZES, numel - G - 1, buffer="output buffer")
    with pytest.raises(ValueError, match="one \\(H, W\\) per offset"):
        PackedLayout.packed([])
    # as_layout: a layout stands for offsets with hw=None and is taken as it is; anything else about it is checked
    assert ragged.as_layout(gap, None, numel) is gap
    assert ragged.as_layout(offs, SIZES, numel).same_as(gap)
    for args, kw in (((gap, SIZES, numel), {}), ((gap, None, numel + 1), {}), ((gap, None, numel, 3), {}), ((gap, None, numel), {"max_samples": 2})):
        with pytest.raises(ValueError):
            ragged.as_layout(*args, **kw)


def test_packed_layout_is_immutable():
    src_off, src_hw = np.array([0, 30 * 53]), np.array(SIZES[:2])
    lay = PackedLayout(src_off, src_hw, 30 * 53 + 13 * 26)
    with pytest.raises(ValueError):
        lay.offsets[0] = 1
    with pytest.raises(ValueError):
        lay.hw[1, 0] = 12
    for name, value in (("offsets", src_off), ("hw", src_hw), ("numel", 7), ("c", 3), ("other", 1)):
        with pytest.raises(AttributeError):
            setattr(lay, name, value)
    src_off[1], src_hw[0, 0] = 5, 1  # the caller's arrays stay the caller's: writable, and no longer read
    assert lay.offsets.tolist() == [0, 30 * 53] and lay.hw.tolist() == [[30, 53], [13, 26]]


def test_containers_hold_a_layout():
    """The containers keep taking host offsets / hw and show them as read-only properties; on the host nothing is uploaded."""
    total = AREAS[0] + AREAS[1]
    buf = torch.arange(total, dtype=torch.int64).to(torch.uint8)
    gt = native_results.GtBatch(buf, np.array([0, AREAS[0]]), np.array(SIZES[:2]))
    res = native_results.RestoredMasks(buf, None, [0, AREAS[0]], SIZES[:2], torch.tensor([3, 4], dtype=torch.int32))
    sel = native_results.ComponentSelection(buf, None, torch.zeros((2, 4), dtype=torch.int64), gt.layout, None)
    bare = native_results.ComponentSelection(None, None, torch.zeros((2, 4), dtype=torch.int64), [0, AREAS[0]], SIZES[:2])  # mode "label"
    assert bare.layout.numel == total and len(bare) == 2
    assert sel.layout is gt.layout and res.layout.same_as(gt.layout)
    for box in (gt, res, sel):
        assert len(box) == 2 and box.offsets.tolist() == [0, AREAS[0]] and box.hw.tolist() == [[30, 53], [13, 26]]
        with pytest.raises(AttributeError):
            box.offsets = [1, 2]
    assert torch.equal(gt.sample(1), buf[AREAS[0]:].view(13, 26)) and torch.equal(res.sample(1), gt.sample(1))
    assert torch.equal(sel.binary_sample(0), buf[:AREAS[0]].view(30, 53))
    assert gt.stack([1]).shape == (1, 13, 26, 1) and gt.stack([1]).dtype == torch.float32
    with pytest.raises(ValueError, match="one size"):
        gt.stack([0, 1])
    with pytest.raises(ValueError):
        res.binary_sample(0)  # restored without a threshold
    with pytest.raises(ValueError, match="outside"):
        native_results.GtBatch(buf[:-1], [0, AREAS[0]], SIZES[:2])


def test_require_tensor_and_workspace_refuse_on_the_host():
    host = torch.zeros(8, dtype=torch.uint8)
    for t, kw, match in ((host, {}, "CUDA"), (host.float(), {}, "uint8"), (host.view(2, 4), {"ndim": 1}, "1-D"), (host, {"numel": 9}, "9 elements"),
                         (None, {}, "uint8"), (np.zeros(8, np.uint8), {}, "CUDA")):
        with pytest.raises(ValueError, match=match):
            ragged.require_tensor(t, "buf", torch.uint8, **kw)
    with pytest.raises(ValueError, match="uint8/float32"):
        ragged.require_tensor(host.double(), "src", (torch.uint8, torch.float32))
    assert ragged.require_tensor(host, "buf", torch.uint8, 1, 8, cuda=False) is host  # what can be told of a host tensor
    with pytest.raises(ValueError, match="packed like binary"):
        ragged.require_tensor(host, "gt (packed like binary)", torch.uint8, 1, 9, cuda=False)
    for nbytes, align in ((-1, 16), (64, 0), (64, 3), (64, 512), (64, -8)):
        with pytest.raises(ValueError, match="workspace"):
            ragged.workspace(nbytes, align, "cuda")
