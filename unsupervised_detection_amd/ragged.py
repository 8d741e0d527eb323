"""The packed batch: n samples of their own sizes in one 1-D buffer, sample i = H_i x W_i x c elements at element offsets[i]
(DESIGN.md 7.0).  Every ragged kernel family reads it -- the input stage (data.py), restore, connected components and the dense CRF at
native resolution (native_results.py, post_processing.py) -- and this module, below all of them, owns its host side:

  check_packed_tables(offsets, hw, numel, ...)   the one validator of the two tables (no GPU needed)
  PackedLayout                                   the validated, immutable tables with their device copies (one upload per device)
  as_layout(offsets, hw, numel, ...)             what a caller was given -- a PackedLayout, or raw tables to validate -- as a PackedLayout
  PackedSamples                                  base of the containers that hold buffers of one layout (RaggedBatch, RestoredMasks, ...)
  upload_tables / workspace / require_tensor     the small device idioms around a call into the library"""
from __future__ import annotations

import numpy as np
import torch

INT32_MAX = int(np.iinfo(np.int32).max)


def check_ranges(first, length, total, what="sample", where="packed buffer", overlap_ok=False):
    """The range rules of a packed buffer on int64 arrays: every range [first, first + length) inside [0, total), no two sharing an
    element (any order, gaps allowed).  ValueError otherwise."""
    if (first < 0).any() or (first + length > total).any():
        raise ValueError("{} outside the {} (offset + size past its end)".format(what, where))
    order = np.argsort(first, kind="stable")
    if not overlap_ok and (first[order][1:] < (first + length)[order][:-1]).any():
        raise ValueError("{}s overlap in the {}".format(what, where))


def check_packed_tables(offsets, hw, numel, c=1, buffer="packed buffer", overlap_ok=False, max_samples=None):
    """Host validation of the tables of a packed batch (the C entry points do not read device tables): at least one sample and one
    (H, W) per offset, every size at least 1x1 and below 2^31 pixels, every sample of H * W * c elements inside the buffer of `numel`
    elements, no two overlapping (overlap_ok: a read-only buffer may share elements), at most max_samples samples.  Returns (offsets
    int64 [n], hw int32 [n,2]), contiguous, as the kernels read them; raises ValueError."""
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if max_samples is not None and len(off) > max_samples:
        raise ValueError("at most {} samples per call".format(max_samples))
    size = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    if len(off) < 1 or len(size) != len(off) or int(c) < 1:
        raise ValueError("a packed batch needs at least one sample, one channel and one (H, W) per offset")
    if (size < 1).any() or (size > INT32_MAX).any() or (size[:, 0] * size[:, 1] > INT32_MAX).any():
        raise ValueError("sample sizes must be at least 1x1 (and below 2^31 pixels)")
    check_ranges(off, size[:, 0] * size[:, 1] * int(c), int(numel), "sample", buffer, overlap_ok)
    return off, np.ascontiguousarray(size.astype(np.int32))


def upload_tables(arrays, device):
    """Host int arrays -> one pinned buffer -> one non-blocking copy on the current stream; device views in the same order.
    (A pinned block of torch's host allocator is not handed out again before the copy that read it has finished.)"""
    raw = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays]
    pos = np.cumsum([0] + [len(r) for r in raw])
    host = torch.from_numpy(np.concatenate(raw)).pin_memory()
    dev = host.to(device, non_blocking=True)
    return [dev[int(pos[i]):int(pos[i + 1])].view(torch.int64 if a.dtype == np.int64 else torch.int32) for i, a in enumerate(arrays)]


class PackedLayout(object):
    """The tables of one packed batch, validated once (check_packed_tables) and immutable: host offsets int64 [n] and hw int32 [n,2]
    (read-only arrays), numel (elements of the buffer), c (channels), n, max_h, max_w.  device_tables() uploads the two tables on first
    use, unless copies that already exist were adopted (data.RaggedLoader's travel with the pixels)."""
    __slots__ = ("offsets", "hw", "numel", "c", "n", "max_h", "max_w", "_dev")

    def __init__(self, offsets, hw, numel, c=1, buffer="packed buffer", overlap_ok=False):
        off, size = check_packed_tables(offsets, hw, numel, c, buffer, overlap_ok)
        off, size = off.copy(), size.copy()  # the caller's arrays stay writable
        off.setflags(write=False), size.setflags(write=False)
        for name, v in (("offsets", off), ("hw", size), ("numel", int(numel)), ("c", int(c)), ("n", len(off)),
                        ("max_h", int(size[:, 0].max())), ("max_w", int(size[:, 1].max())), ("_dev", {})):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a PackedLayout is immutable")

    @classmethod
    def packed(cls, hw, c=1):
        """The layout of samples of sizes hw [n,2] stored back to back."""
        size = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
        end = np.cumsum(size[:, 0] * size[:, 1] * int(c))
        return cls(np.concatenate([[0], end[:-1]]), size, int(end[-1]) if len(end) else 0, c)

    def __len__(self):
        return self.n

    def __array__(self, dtype=None, copy=None):
        """np.asarray(layout): the sizes [n,2] -- what a function that takes `native_hw` reads."""
        return self.hw if dtype is None else self.hw.astype(dtype)

    def view(self, buf, i):
        """Sample i of the packed buffer `buf` as a view: [H_i, W_i], or [H_i, W_i, c] with c > 1."""
        H, W = (int(v) for v in self.hw[i])
        o = int(self.offsets[i])
        return buf[o:o + H * W * self.c].view((H, W) if self.c == 1 else (H, W, self.c))

    def same_as(self, other, scale=1):
        """True where this layout is `other`'s with `scale` times the elements per pixel: the same sizes in the same order, offsets,
        channels and buffer length times scale (rgb frames beside their one-channel masks: scale=3)."""
        if self is other and scale == 1:
            return True
        return (self.numel == scale * other.numel and self.c == scale * other.c and np.array_equal(self.hw, other.hw) and
                np.array_equal(self.offsets, scale * other.offsets))

    def adopt_device_tables(self, d_off, d_hw):
        """Device copies of these tables that already exist (in stream order with the buffer they came with): device_tables() hands them
        out on their device and uploads nothing there."""
        if d_off.numel() != self.n or d_hw.numel() != 2 * self.n or d_off.dtype != torch.int64 or d_hw.dtype != torch.int32:
            raise ValueError("device tables do not match the host tables")
        self._dev.setdefault(d_off.device, (d_off, d_hw))

    def device_tables(self, device):
        """(offsets int64 [n], hw int32 [n,2]) on `device`: uploaded once per layout and device (upload_tables), then reused."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = tuple(upload_tables([self.offsets, self.hw], device))
            torch.cuda.current_stream(device).synchronize()  # once per layout: a later call may run on another stream
        return self._dev[device]


def as_layout(offsets, hw, numel, c=1, buffer="packed buffer", overlap_ok=False, max_samples=None) -> PackedLayout:
    """The layout a caller described: a PackedLayout given as `offsets` (with hw=None) is taken as it is -- it was validated when it was
    built, only its buffer length is compared -- and raw tables are validated into a new one."""
    given = isinstance(offsets, PackedLayout)
    layout = offsets if given else PackedLayout(offsets, hw, numel, c, buffer, overlap_ok)
    if given and (hw is not None or layout.numel != int(numel) or layout.c != int(c)):
        raise ValueError("a PackedLayout stands for offsets and hw (hw=None) of a {} of its own {} elements and {} channel(s)".format(
            buffer, layout.numel, layout.c))
    if max_samples is not None and layout.n > max_samples:
        raise ValueError("at most {} samples per call".format(max_samples))
    return layout


class PackedSamples(object):
    """Base of the containers of packed buffers: one `layout` for all their buffers, which live on `device`."""

    def __init__(self, layout, device):
        self.layout, self.device = layout, device

    offsets = property(lambda self: self.layout.offsets)
    hw = property(lambda self: self.layout.hw)
    dev_offsets = property(lambda self: self.layout.device_tables(self.device)[0])
    dev_hw = property(lambda self: self.layout.device_tables(self.device)[1])

    def __len__(self):
        return self.layout.n

    def _view(self, buf, i):
        return self.layout.view(buf, i)

    def stack(self, idx):
        """[k,H,W,1] float32 0 / 1 tensor of the binary masks of samples idx (all of one size): what the metrics kernels take."""
        idx = list(idx)
        if len({tuple(int(v) for v in self.hw[i]) for i in idx}) != 1:
            raise ValueError("stack: the samples must be of one size")
        return torch.stack([self.binary_sample(i) for i in idx]).to(torch.float32).unsqueeze(-1).contiguous()


def workspace(nbytes, align, device):
    """The workspace of a `udet_*_workspace_bytes` call: a uint8 device tensor of at least nbytes bytes whose address is a multiple of
    align (a power of two up to 256: the device allocator's own granule is larger)."""
    nbytes, align = int(nbytes), int(align)
    if nbytes < 0 or align < 1 or align > 256 or align & (align - 1):
        raise ValueError("workspace: nbytes >= 0 and an alignment that is a power of two in 1..256")
    ws = torch.empty(max(nbytes, align), dtype=torch.uint8, device=device)
    if ws.data_ptr() % align:
        raise RuntimeError("workspace: the device allocator returned an address that is no multiple of {}".format(align))
    return ws


def require_tensor(t, name, dtype, ndim=None, numel=None, device=None, cuda=True):
    """ValueError unless t is a contiguous CUDA(HIP) tensor of `dtype` (one dtype or a tuple), and of ndim dimensions, numel elements
    and on `device` where these are given.  cuda=False: only what can be told of a host tensor too (type, dtype, dimensions, elements).
    Returns t."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    ok = isinstance(t, torch.Tensor) and t.dtype in dtypes and (ndim is None or t.dim() == ndim) and (numel is None or t.numel() == numel)
    if ok and cuda:
        ok = t.is_cuda and t.is_contiguous() and (device is None or t.device == device)
    if not ok:
        raise ValueError("{} must be a contiguous {}{} CUDA(HIP) tensor{}{}".format(
            name, "" if ndim is None else "{}-D ".format(ndim), "/".join(str(d).replace("torch.", "") for d in dtypes),
            "" if numel is None else " of {} elements".format(numel), "" if device is None else " on {}".format(device)))
    return t
