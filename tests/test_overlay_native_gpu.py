"""GPU: udet_overlay_native_ragged (csrc/visualize.hip) through visualize.overlay_native -- exact equality with a numpy restatement
written here (float32 blend with np.rint, scipy's erosion), with visualize.overlay_mask at the frame's own size as a second witness,
on packed batches with guard bytes, and the error paths of the C entry point."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# degenerate frames | smaller than a tile and its halo | one past a tile edge (32 x 64) | several tiles
SIZES = [(1, 1), (1, 70), (67, 1), (9, 13), (33, 65), (40, 150)]
BLOBS = (2, 3, 4, 5)  # the samples whose mask has an inside and an outside
GUARD = 0xA5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return True


# ------------------------------------------------------------------------------------------------------------ restatement ----
def overlay_np(img, mask, alpha=0.5, beta=0.4, colour=(0, 255, 0), edge=2, edge_colour=(255, 255, 255)):
    """include/udet.h, udet_overlay_native_ragged: two float32 products and a float32 sum, np.rint, saturation; the contour is
    fg & ~binary_erosion(fg, ones((2 edge + 1, 2 edge + 1)), border_value=1), written unblended."""
    from scipy.ndimage import binary_erosion
    fg = mask != 0
    m = np.zeros(img.shape, np.float32)
    m[fg] = np.asarray(colour, np.float32)
    with np.errstate(over="ignore"):
        a, b = img.astype(np.float32) * np.float32(alpha), m * np.float32(beta)
        t = np.rint(a + b)
    assert a.dtype == b.dtype == t.dtype == np.float32
    out = np.clip(t, 0, 255).astype(np.uint8)
    contour = np.zeros_like(fg)
    if edge >= 1:
        contour = fg & ~binary_erosion(fg, np.ones((2 * edge + 1, 2 * edge + 1), bool), border_value=1)
        out[contour] = np.asarray(edge_colour, np.uint8)
    return out, contour


def ellipse(h, w, cy, cx, ry, rx):
    y, x = np.mgrid[:h, :w]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def make_samples():
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    images[5].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)  # every byte value, the odd ones (ties of v * 0.5) among them
    masks = [np.zeros(hw, np.uint8) for hw in SIZES]
    masks[0][:] = 1                 # 1 x 1: all foreground (no background inside the frame: no contour)
    #        1 x 70: all background
    masks[2][5:41] = 255            # 67 x 1: a run of rows; any non-zero byte is foreground
    masks[3][0:6, 0:9] = 1          # 9 x 13: a rectangle on the top and the left border
    masks[4][:] = 1
    masks[4][32, 64] = 0            # 33 x 65: one background pixel one past the tile's edge and corner: tile (0, 0)'s contour comes from tile (1, 1)
    masks[5][ellipse(40, 150, 15, 40, 10, 25)] = 1
    masks[5][0:7, 60:71] = 1        # on the top border, joined to the ellipse
    masks[5][25:40, 100:150] = 7    # on the bottom and the right border ...
    masks[5][32, 128] = 0           # ... with a hole on a tile corner
    return images, masks


class Packed(object):
    """Frames and masks packed by hand: masks at element offsets `offsets`, frames at three times those, guard bytes elsewhere."""

    def __init__(self, images, masks, offsets=None, total=None, order=None):
        from unsupervised_detection_amd.ragged import PackedLayout
        order = list(range(len(images))) if order is None else order
        self.images, self.masks = [images[i] for i in order], [masks[i] for i in order]
        hw = [m.shape for m in self.masks]
        if offsets is None:
            self.layout = PackedLayout.packed(hw)
        else:
            self.layout = PackedLayout(offsets, hw, total)
        off, total = self.layout.offsets, self.layout.numel
        self.frames_layout = PackedLayout(3 * off, hw, 3 * total, 3)
        img, msk = np.full(3 * total, GUARD, np.uint8), np.full(total, GUARD, np.uint8)
        for o, im, m in zip(off, self.images, self.masks):
            img[3 * o:3 * o + im.size] = im.reshape(-1)
            msk[o:o + m.size] = m.reshape(-1)
        self.data = torch.from_numpy(img).cuda()
        self.binary = torch.from_numpy(msk).cuda()

    class _Frames(object):
        pass

    @property
    def frames(self):
        f = self._Frames()
        f.data, f.layout = self.data, self.frames_layout
        return f


@pytest.fixture(scope="module")
def samples(gpu):
    images, masks = make_samples()
    return images, masks, Packed(images, masks)


# ----------------------------------------------------------------------------------------------------------------- tests ----
def test_the_inputs_exercise_what_they_are_meant_to():
    images, masks = make_samples()
    assert len(np.unique(np.concatenate([im.reshape(-1) for im in images]))) == 256
    assert masks[0].all() and not masks[1].any()
    for e in (1, 2):
        for i in BLOBS:
            fg = masks[i] != 0
            _, contour = overlay_np(images[i], masks[i], edge=e)
            assert contour.any() and not (contour & ~fg).any() and (fg & ~contour).any(), (i, e)  # a non-empty strict subset of the foreground
    _, c = overlay_np(images[4], masks[4], edge=1)
    assert c[31, 63] and c[31, 64] and c[32, 63] and not c[32, 64] and c.sum() == 3  # decided across the tile's edge and corner
    _, c = overlay_np(images[3], masks[3], edge=2)
    assert not c[0, :6].any() and not c[:3, 0].any() and c[5, :9].all() and c[:6, 8].all()  # no line along the frame border
    _, c = overlay_np(images[0], masks[0], edge=2)
    assert not c.any()


@pytest.mark.parametrize("edge", [0, 1, 2, 8])
def test_against_the_restatement(samples, edge):
    from unsupervised_detection_amd.visualize import overlay_native
    images, masks, p = samples
    got = overlay_native(p.frames, p, edge=edge)
    assert len(got) == len(SIZES)
    for i, (im, m) in enumerate(zip(images, masks)):
        want, _ = overlay_np(im, m, edge=edge)
        g = got.sample(i)
        assert g.dtype == torch.uint8 and tuple(g.shape) == im.shape
        assert np.array_equal(g.cpu().numpy(), want), (edge, i, SIZES[i])


@pytest.mark.parametrize("kw", [dict(alpha=0.75, beta=0.3, colour=(255, 0, 128), edge=1, edge_colour=(1, 2, 3)),
                                dict(alpha=1.0, beta=1.0, colour=(200, 255, 90), edge=3, edge_colour=(0, 0, 0)),   # saturates
                                dict(alpha=3.0e38, beta=0.0, colour=(9, 9, 9), edge=0),                            # the product overflows
                                dict(alpha=0.0, beta=0.123, colour=(255, 255, 255), edge=2)])
def test_other_weights_and_colours(samples, kw):
    from unsupervised_detection_amd.visualize import overlay_native
    images, masks, p = samples
    got = overlay_native(p.frames, p, **kw)
    sat = False
    for i, (im, m) in enumerate(zip(images, masks)):
        want, _ = overlay_np(im, m, **kw)
        sat = sat or (want == 255).any()
        assert np.array_equal(got.sample(i).cpu().numpy(), want), (kw, i)
    if kw["alpha"] >= 1.0:
        assert sat


def test_overlay_mask_is_a_second_witness(gpu):
    """edge = 0 and the defaults: visualize.overlay_mask at oh = h, ow = w (where its resize is the identity: test_visualize_gpu.py) on
    the same bytes and a mask that is not complemented."""
    from unsupervised_detection_amd.visualize import overlay_mask, overlay_native
    rng = np.random.default_rng(5)
    for h, w in ((33, 65), (40, 150)):
        v = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        image = ((v + 0.25) / 255.0 - 0.5).astype(np.float32)
        assert np.array_equal(np.trunc((image + np.float32(0.5)) * np.float32(255)), v)  # postprocess_image gives the bytes back
        m = ellipse(h, w, h / 2, w / 2, h / 3, w / 3).astype(np.uint8)  # away from the border: never complemented
        ref = overlay_mask(torch.from_numpy(image[None]).cuda(), torch.from_numpy(m.astype(np.float32)[None, ..., None]).cuda(), (h, w))
        p = Packed([v], [m])
        got = overlay_native(p.frames, p, edge=0)
        assert torch.equal(got.sample(0), ref[0]), (h, w)


def test_guards_order_and_repeatability(samples):
    from unsupervised_detection_amd.visualize import overlay_native
    images, masks, p = samples
    base = overlay_native(p.frames, p, edge=2)
    again = overlay_native(p.frames, p, edge=2)
    assert torch.equal(base.data, again.data)
    # odd offsets, guard bytes before, between and after the samples, another order
    order = [5, 0, 3, 1, 4, 2]
    sizes = [SIZES[i][0] * SIZES[i][1] for i in order]
    offsets, at = [], 5
    for k, s in enumerate(sizes):
        offsets.append(at)
        at += s + (3, 1, 8, 2, 5, 9)[k]
    assert {o % 4 for o in offsets} == {0, 1, 2, 3} and any(o % 2 for o in offsets)
    q = Packed(images, masks, offsets, at, order)
    out = torch.full((3 * at,), GUARD, dtype=torch.uint8, device="cuda")
    got = overlay_native(q.frames, q, edge=2, out=out)
    assert got.data.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    written = np.zeros(3 * at, bool)
    for k, i in enumerate(order):
        o, n = 3 * offsets[k], 3 * sizes[k]
        written[o:o + n] = True
        assert np.array_equal(host[o:o + n], base.sample(i).cpu().numpy().reshape(-1)), (k, i)  # as inside the packed batch
    assert (~written).sum() == 3 * (5 + 3 + 1 + 8 + 2 + 5 + 9) and (host[~written] == GUARD).all()
    # a sample alone, in a buffer whose address is not a multiple of 4 (the byte-by-byte path)
    for i in (3, 4):
        alone = Packed([images[i]], [masks[i]])
        assert torch.equal(overlay_native(alone.frames, alone, edge=2).sample(0), base.sample(i)), i
        shifted = torch.full((alone.data.numel() + 1,), GUARD, dtype=torch.uint8, device="cuda")
        shifted[1:] = alone.data
        f = Packed._Frames()
        f.data, f.layout = shifted[1:], alone.frames_layout
        assert f.data.data_ptr() % 4 == 1
        assert torch.equal(overlay_native(f, alone, edge=2).sample(0), base.sample(i)), i


def test_wrapper_refuses_before_the_device_is_touched(samples):
    from unsupervised_detection_amd.visualize import overlay_native
    images, masks, p = samples
    for kw in (dict(edge=9), dict(edge=-1), dict(edge=1.5), dict(alpha=-0.1), dict(beta=float("nan")), dict(alpha=float("inf")),
               dict(colour=(0, 256, 0)), dict(edge_colour=(1, 2)), dict(out=p.data), dict(out=torch.zeros(5, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            overlay_native(p.frames, p, **kw)
    other = Packed(images[:2], masks[:2])
    with pytest.raises(ValueError, match="packed like the masks"):
        overlay_native(other.frames, p)


def test_c_entry_point_errors_leave_the_output_untouched(samples):
    from unsupervised_detection_amd._ffi import lib
    images, masks, p = samples
    total = p.layout.numel
    out = torch.full((3 * total,), GUARD, dtype=torch.uint8, device="cuda")
    d_off, d_hw = p.layout.device_tables(out.device)
    ok = dict(image=p.data.data_ptr(), mask=p.binary.data_ptr(), n=p.layout.n, offsets=d_off.data_ptr(), hw=d_hw.data_ptr(),
              max_h=p.layout.max_h, max_w=p.layout.max_w, total=total, alpha=0.5, beta=0.4, mask_rgb=0x00FF00, edge=2, edge_rgb=0xFFFFFF,
              out=out.data_ptr())

    def call(**change):
        a = dict(ok, **change)
        return lib.udet_overlay_native_ragged(a["image"], a["mask"], a["n"], a["offsets"], a["hw"], a["max_h"], a["max_w"], a["total"],
                                              a["alpha"], a["beta"], a["mask_rgb"], a["edge"], a["edge_rgb"], a["out"],
                                              torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")
    for change in (dict(n=0), dict(n=65536), dict(image=None), dict(mask=None), dict(offsets=None), dict(hw=None), dict(out=None),
                   dict(max_h=0), dict(max_w=0), dict(max_w=-3), dict(edge=-1), dict(alpha=-1.0), dict(alpha=nan), dict(alpha=inf),
                   dict(beta=-1e-9), dict(beta=nan), dict(beta=-inf), dict(beta=inf)):
        assert call(**change) == -5 and b"overlay_native_ragged" in lib.udet_last_error(), change  # UDET_ERR_ARG
    assert call(edge=9) == -4 and b"UDET_OVERLAY_MAX_EDGE" in lib.udet_last_error()  # UDET_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out == GUARD).all()
    assert call() == 0
    torch.cuda.synchronize()
    for i, (im, m) in enumerate(zip(images, masks)):
        assert np.array_equal(p.frames_layout.view(out, i).cpu().numpy(), overlay_np(im, m)[0]), i
