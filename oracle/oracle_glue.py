"""Plain restatements of the step's glue, loss-tail and optimizer operations (csrc/elementwise.hip), straight from their definitions.

Two forms where both make sense:
  *_f32  float32 with the kernel's documented operation order.  elementwise.hip is built without FMA contraction, so copies, packs,
         share, fold in its fixed order (x0 + x1) + x2, emit_du for leaky / none, the resize forward and the clip are held bit for bit.
  *_f64  float64 for everything with a transcendental, a division chain or a reduction; gradients are torch.autograd through the float64
         forward composite, never a second hand-derived formula.
tests/test_glue_oracle.py holds the forms to each other on the CPU; tests/test_glue_gpu.py and tests/test_stage_ops_gpu.py hold the kernels
to them.  The case builders at the end are shared by both, so that the tolerances measured on the CPU are measured on the GPU tests' own
inputs (TOL)."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import oracle_torch as O

ACT_NONE, ACT_LEAKY, ACT_ELU = 0, 1, 2
SENTINEL = -7777.25  # fills everything a kernel must not write


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# copies and packs (bit-exact float32)
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_pwc_input(i1, i2):
    """model_pwcnet.py:39-56 adapt_x: [2P, 4] = [img + 0.5 | 0] for the stacked images; i1, i2 [P, 3]."""
    x = torch.cat([i1, i2], 0) + torch.tensor(0.5, dtype=i1.dtype)
    return torch.cat([x, torch.zeros(x.shape[0], 1, dtype=i1.dtype)], 1)


def pack_imgin(img, ncalls):
    """nets.py:57: [ncalls * P, 4] = [img | 0] once per recover call; img [P, 3]."""
    one = torch.cat([img, torch.zeros(img.shape[0], 1, dtype=img.dtype)], 1)
    return one.repeat(ncalls, 1)


def share(buf, P, coff, C, copies):
    """rows [kP, (k+1)P) of the window [coff, coff + C) <- rows [0, P), k = 1..copies-1; buf [>= copies * P, ld]"""
    out = buf.clone()
    for k in range(1, copies):
        out[k * P:(k + 1) * P, coff:coff + C] = buf[:P, coff:coff + C]
    return out


def fold(buf, P, coff, C, copies):
    """rows [0, P) of the window <- (x0 + x1) + x2 in that order; the source rows stay"""
    out = buf.clone()
    acc = buf[:P, coff:coff + C].clone()
    for k in range(1, copies):
        acc = acc + buf[k * P:(k + 1) * P, coff:coff + C]
    out[:P, coff:coff + C] = acc
    return out


def act_derivative_from_output(a, act, alpha):
    """act'(pre-activation) expressed by the stored OUTPUT a: 1 where a > 0; else alpha (leaky), a + 1 (ELU: exp(x) = elu(x) + 1), 1 (none)"""
    one = torch.ones_like(a)
    neg = {ACT_NONE: one, ACT_LEAKY: one * alpha, ACT_ELU: a + 1}[act]
    return torch.where(a > 0, one, neg)


def emit_du(d, a, coff, C, act, alpha, u0):
    """u = d * act'(a) on the window, u0 elsewhere; dtype of d (float32: kernel order, one multiply; float64: reference)"""
    u = u0.clone().to(d.dtype)
    w = slice(coff, coff + C)
    u[:, w] = d[:, w] * act_derivative_from_output(a[:, w], act, torch.tensor(alpha, dtype=torch.float32).to(d.dtype))
    return u


# ---------------------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------------------
def resize_fwd_f32(x, oh, ow, mul=1.0, div=1.0):
    """O.resize_bilinear_legacy(x) * mul / div in float32, the kernel's order: the lerps, then * mul, then / div unless div == 1.
    (Same size: scale 1, every lerp weight 0 -- the kernel has no shortcut, the value is x.)"""
    assert x.dtype == torch.float32
    v = O.resize_bilinear_legacy(x, oh, ow) * torch.tensor(mul, dtype=torch.float32)
    return v / torch.tensor(div, dtype=torch.float32) if div != 1.0 else v


def _resize_no_shortcut(x, oh, ow):
    if x.shape[1] == oh and x.shape[2] == ow:
        return x * 1.0
    return O.resize_bilinear_legacy(x, oh, ow)


def resize_bwd_f64(dy, h, w):
    """adjoint of the legacy resize [n,h,w,c] -> dy's grid: float64 autograd of O.resize_bilinear_legacy"""
    n, oh, ow, c = dy.shape
    x = torch.zeros(n, h, w, c, dtype=torch.float64, requires_grad=True)
    y = _resize_no_shortcut(x, oh, ow)
    g, = torch.autograd.grad(y, [x], dy.double())
    return g


def interp_matrix(in_size, out_size):
    """[out, in] float64: row o holds 1 - t at lower(o) and t at upper(o) (added when both are the same source pixel)"""
    lo, hi, t = O._legacy_interp_table(in_size, out_size)
    A = np.zeros((out_size, in_size))
    for o in range(out_size):
        A[o, lo[o]] += 1.0 - float(t[o])
        A[o, hi[o]] += float(t[o])
    return torch.from_numpy(A)


def resize_bwd_matrix(dy, h, w):
    """the same adjoint written out: dx = Ay^T dy Ax per sample and channel (the definition the gather kernel implements)"""
    n, oh, ow, c = dy.shape
    return torch.einsum("oi,nopc,pj->nijc", interp_matrix(h, oh), dy.double(), interp_matrix(w, ow))


# ---------------------------------------------------------------------------------------------------------------------------------
# flow standardisation / generator input
# ---------------------------------------------------------------------------------------------------------------------------------
def flow_standardise_f32(f):
    """kernel order: mean and population variance accumulated in double (var = E[x^2] - mean^2), each rounded to float32,
    std = sqrtf(var), then (f - mean) / std in float32; f [B, HW, 2] float32"""
    d = f.double()
    mean = d.mean(1, keepdim=True)
    var = (d * d).mean(1, keepdim=True) - mean * mean
    return (f - mean.float()) / torch.sqrt(var.float())


def flow_standardise_f64(f):
    B, HW, _ = f.shape
    return O.preprocess_flow_batch(f.double().view(B, 1, HW, 2)).view(B, HW, 2)


def gen_input_f64(img, f):
    """[B, HW, 8] = [image (3), standardised flow (2), 0, 0, 0]   (nets.py:14, adversarial_learner.py:99-105)"""
    B, HW, _ = f.shape
    return torch.cat([img.double(), flow_standardise_f64(f), torch.zeros(B, HW, 3, dtype=torch.float64)], 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# mask + recover inputs and their backward (nets.py:38-41,50-52; adversarial_learner.py:107-131)
# ---------------------------------------------------------------------------------------------------------------------------------
def mask_composite_f64(l01, f):
    """l01 [P, 2] logits, f [P, 2] -> mask [P], fin [3, P, 4] = [f (1-m), 1, 1-m], [f m, 1, m], [0, 0, 1, 0]   (float64, differentiable)"""
    l01, f = l01.double(), f.double()
    m = torch.softmax(l01 / 10.0, dim=1)[:, 0]
    cm = 1.0 - m
    one, zero = torch.ones_like(m), torch.zeros_like(m)
    c0 = torch.stack([f[:, 0] * (1.0 - m), f[:, 1] * (1.0 - m), one, 1.0 - m], 1)
    c1 = torch.stack([f[:, 0] * (1.0 - cm), f[:, 1] * (1.0 - cm), one, 1.0 - cm], 1)
    c2 = torch.stack([zero, zero, one, zero], 1)
    return m, torch.stack([c0, c1, c2], 0)


def mask_composite_f32(l01, f):
    """the kernel's order in float32: l / 10, subtract the max, expf, e0 / (e0 + e1); a0 = 1 - m, a1 = 1 - (1 - m)"""
    assert l01.dtype == torch.float32 and f.dtype == torch.float32
    l0, l1 = l01[:, 0] / 10.0, l01[:, 1] / 10.0
    mx = torch.maximum(l0, l1)
    e0, e1 = torch.exp(l0 - mx), torch.exp(l1 - mx)
    m = e0 / (e0 + e1)
    cm = 1.0 - m
    a0, a1 = 1.0 - m, 1.0 - cm
    one, zero = torch.ones_like(m), torch.zeros_like(m)
    c0 = torch.stack([f[:, 0] * a0, f[:, 1] * a0, one, a0], 1)
    c1 = torch.stack([f[:, 0] * a1, f[:, 1] * a1, one, a1], 1)
    return m, torch.stack([c0, c1, torch.stack([zero, zero, one, zero], 1)], 0)


def mask_bwd_f64(l01, f, dmask, dfin):
    """d/dlogits of <dmask, mask> + <dfin[0], fin[0]> + <dfin[1], fin[1]>: autograd through mask_composite_f64 -> [P, 2]"""
    l = l01.double().clone().requires_grad_(True)
    m, fin = mask_composite_f64(l, f)
    s = (dmask.double() * m).sum() + (dfin[:2].double() * fin[:2]).sum()
    g, = torch.autograd.grad(s, [l])
    return g


def mask_bwd_f32(mask, f, dmask, dfin):
    """the kernel's order from the STORED float32 mask: dm = dmask - (g0.f + g0[3]) + (g1.f + g1[3]); d0 = dm m (1 - m) / 10"""
    g0, g1 = dfin[0], dfin[1]
    dm = dmask - ((g0[:, 0] * f[:, 0] + g0[:, 1] * f[:, 1]) + g0[:, 3])
    dm = dm + ((g1[:, 0] * f[:, 0] + g1[:, 1] * f[:, 1]) + g1[:, 3])
    d0 = dm * mask * (1.0 - mask) / 10.0
    return torch.stack([d0, -d0], 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# losses (adversarial_learner.py:141-204)
# ---------------------------------------------------------------------------------------------------------------------------------
LOSS_KEYS = ("generator", "recover", "red_rate", "red_rate_compl", "reconstruction_loss", "reconstruction_compl_loss",
             "denominator_red_rate", "denominator_red_rate_compl")


def generator_loss_of_sums(R, D, Rc, Dc):
    """the generator loss as a function of the four per-sample sums (D, Dc with epsilon added): mean(1 - R / D) + mean(1 - Rc / Dc)"""
    return (1.0 - R / D).mean() + (1.0 - Rc / Dc).mean()


def losses(flow, mask, pred3, cbn, eps):
    """the eight losses and the per-sample sums, in the dtype of the inputs (float64: the reference; differentiable)"""
    B = flow.shape[0]
    p, pc, pi = pred3[:B], pred3[B:2 * B], pred3[2 * B:]
    cm = 1.0 - mask
    R = O.charbonnier_loss(flow, p, mask, cbn)
    Rc = O.charbonnier_loss(flow, pc, cm, cbn)
    prior = O.charbonnier_loss(flow, pi, torch.ones_like(flow), cbn)
    D = O.charbonnier_loss(flow, pi, mask, cbn) + eps
    Dc = O.charbonnier_loss(flow, pi, cm, cbn) + eps
    npx = float(flow.shape[1] * flow.shape[2] * B)
    red, redc = (1.0 - R / D).mean(), (1.0 - Rc / Dc).mean()
    out = {"generator": red + redc, "recover": (R.sum() + Rc.sum() + prior.sum()) / npx, "red_rate": red, "red_rate_compl": redc,
           "reconstruction_loss": R[0], "reconstruction_compl_loss": Rc[0], "denominator_red_rate": D[0], "denominator_red_rate_compl": Dc[0]}
    return out, (R, D, Rc, Dc)


def coef_f64(flow, mask, pred3, cbn, eps):
    """[B, 4] = d generator / d (R_b, D_b, Rc_b, Dc_b): float64 autograd through generator_loss_of_sums at the float64 sums"""
    _, sums = losses(flow.double(), mask.double(), pred3.double(), cbn, eps)
    leaves = [s.detach().clone().requires_grad_(True) for s in sums]
    g = torch.autograd.grad(generator_loss_of_sums(*leaves), leaves)
    return torch.stack(g, 1)


def coef_f32(flow, mask, pred3, cbn, eps):
    """the kernel's formulas in float32: -1 / (B D), R / (B D D), -1 / (B Dc), Rc / (B Dc Dc) on float32 sums"""
    _, (R, D, Rc, Dc) = losses(flow, mask, pred3, cbn, eps)
    B = float(flow.shape[0])
    return torch.stack([-1.0 / (B * D), R / (B * D * D), -1.0 / (B * Dc), Rc / (B * Dc * Dc)], 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# train_op's escape rule (loss_utils.py:19-26) and the clipped Adam apply
# ---------------------------------------------------------------------------------------------------------------------------------
def mean_of_means(grads: dict):
    """mean over the variables of mean |g_v| -- what O.clip_or_noise compares with 1e-5 (float64)"""
    return float(torch.stack([g.double().abs().mean() for g in grads.values()]).mean())


def global_absmean(grads: dict):
    """the statistic a wrong kernel could take instead: the mean of |g| over all elements"""
    return float(sum(g.double().abs().sum() for g in grads.values()) / sum(g.numel() for g in grads.values()))


def flag_stage_f32(var_sums, lens):
    """grad_flag_kernel's float32 order from the per-variable sums: s += sum_v / len_v sequentially, then s / nvars"""
    s = np.float32(0)
    for v, n in zip(var_sums, lens):
        s = np.float32(s + np.float32(np.float32(v) / np.float32(n)))
    return np.float32(s / np.float32(len(lens)))


THRESH = np.float32(1e-5)


def table_lens(table):
    return [int(np.prod(shape)) for _, shape, _ in table]


def flat_from_constants(table, consts):
    total = table[-1][2] + table_lens(table)[-1]
    g = torch.zeros(total)
    for (_, _, off), n, c in zip(table, table_lens(table), consts):
        g[off:off + n] = float(c)
    return g


def as_dict(flat, table):
    return {name: flat[off:off + n] for (name, _, off), n in zip(table, table_lens(table))}


def rule_cases(table):
    """Two gradients with per-variable constants (powers of two, or zero) that separate the mean of means from the global mean of |g|:
    'means_high'  the short half of the variables set, the long ones zero: mean of means >= 4e-5, global mean <= 2.5e-6 -> no escape;
    'means_low'   the longest variable set, the rest zero:                 mean of means < 1e-5 < global mean -> escape.
    For ANY gradient, global mean = sum_v len_v mean_v / total <= max_len * nvars / total * (mean of means): the two statistics cannot be
    further apart in this direction than that ratio (rule_ratio_bound: 6.9 for the generator, 14.9 for the recover net), so a factor of 4
    on each side (ratio 16) does not exist here; the power of two with the widest margin on the narrower side is taken (>= 2 on each).
    Returns {name: (per-variable constants, mean of means, global mean)}; tests assert the inequalities before they use a case."""
    lens = np.array(table_lens(table), dtype=np.float64)
    nv, total = len(lens), lens.sum()
    order = np.argsort(lens, kind="stable")
    out = {}
    small = np.zeros(nv, bool)
    small[order[:nv // 2]] = True
    c = 2.0 ** math.ceil(math.log2(4e-5 * nv / small.sum()))
    out["means_high"] = (np.where(small, c, 0.0), c * small.sum() / nv, c * lens[small].sum() / total)
    big = np.zeros(nv, bool)
    big[order[-1]] = True
    margin = lambda c: min(c * lens[big].sum() / total / 1e-5, 1e-5 / (c / nv))  # noqa: E731
    c = max((2.0 ** e for e in range(-30, 0)), key=margin)
    out["means_low"] = (np.where(big, c, 0.0), c / nv, c * lens[big].sum() / total)
    return out


def rule_ratio_bound(table):
    """the largest possible (global mean of |g|) / (mean of means) over all gradients: max_len * nvars / total"""
    lens = table_lens(table)
    return max(lens) * len(lens) / sum(lens)


def exact_threshold_gradient(table):
    """A gradient whose mean of means comes out as exactly float32(1e-5) in the kernels' float32 order: one non-zero element y in
    variable 0 (every sum is exact), searched so that fl(fl(y / len_0) / nvars) == 1e-5f.  Returns (flat gradient, replayed value)."""
    lens = table_lens(table)
    nv, n0 = np.float32(len(lens)), np.float32(lens[0])
    x = np.float32(THRESH * nv)
    for _ in range(64):  # the per-variable mean x with fl(x / nvars) == 1e-5f
        q = np.float32(x / nv)
        if q == THRESH:
            break
        x = np.nextafter(x, np.float32(np.inf) if q < THRESH else np.float32(-np.inf), dtype=np.float32)
    y = np.float32(x * n0)
    for _ in range(64):
        q = np.float32(y / n0)
        if q == x:
            break
        y = np.nextafter(y, np.float32(np.inf) if q < x else np.float32(-np.inf), dtype=np.float32)
    g = torch.zeros(table[-1][2] + lens[-1])
    g[table[0][2]] = float(y)
    return g, flag_stage_f32([y] + [0.0] * (len(lens) - 1), lens)


def adam_lr_t(t, lr=1e-4, b1=0.9, b2=0.999):
    """udet_adam_step's float64 closed form, rounded to float32 as the kernel receives it"""
    return float(np.float32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))


def adam_f64(w, g, m, v, t, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8):
    """one apply of O.TFAdam in float64 with the beta powers of apply number t -> (w, m, v)"""
    opt = O.TFAdam(lr, b1, b2, eps)
    opt.b1p, opt.b2p = b1 ** t, b2 ** t
    opt.m["x"], opt.v["x"] = m.double().clone(), v.double().clone()
    p = {"x": w.double().clone()}
    opt.apply(p, {"x": g.double()})
    return p["x"], opt.m["x"], opt.v["x"]


def adam_f32(w, g, m, v, t, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8):
    """adam_kernel's order in float32: m + (g - m)(1 - b1); v + (g g - v)(1 - b2); w - lr_t m / (sqrt(v) + eps)"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    mi = m + (g - m) * (f(1.0) - f(b1))
    vi = v + (g * g - v) * (f(1.0) - f(b2))
    return w - f(adam_lr_t(t, lr, b1, b2)) * mi / (torch.sqrt(vi) + f(eps)), mi, vi


def clip_f32(g, clip):
    return g.clamp(-clip, clip)


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU tests' own inputs (shared with the CPU test that measures TOL on them)
# ---------------------------------------------------------------------------------------------------------------------------------
SPATIAL = ((1, 1), (3, 5), (1, 257), (257, 1), (7, 9), (6, 12), (33, 40))


def mask_case(P, seed):
    """logits [P, 8] (channels 2..7 sentinel), flow [P, 2]; pixel 0 has equal logits (m = 0.5), pixels 1 / 2 logits of +-2000 (m = 1 / 0)"""
    g = gen(seed)
    logits = torch.full((P, 8), SENTINEL)
    logits[:, :2] = torch.randn(P, 2, generator=g) * 30.0
    logits[0, :2] = 3.25
    if P > 1:
        logits[1, 0], logits[1, 1] = 2000.0, -2000.0
    if P > 2:
        logits[2, 0], logits[2, 1] = -2000.0, 2000.0
    return logits, torch.randn(P, 2, generator=g)


def mask_bwd_case(P, seed):
    logits, f = mask_case(P, seed)
    g = gen(seed + 100)
    return logits, f, torch.randn(P, generator=g), torch.randn(3, P, 4, generator=g)


def emit_case(P, ld, seed):
    """d, a [P, ld]: a on both sides of zero, exactly zero in places, never below -1 (an ELU output)"""
    g = gen(seed)
    d = torch.randn(P, ld, generator=g)
    a = torch.randn(P, ld, generator=g)
    a = torch.where(a < 0, torch.expm1(a), a)
    a.view(-1)[::5] = 0.0
    return d, a


ADAM_CLIP = 0.2


def adam_case(n, seed):
    """w, g, m, v [n]: g holds exactly +-clip, +-(clip + 1 ulp), 0 and 1e-20 at its front (cyclically), the rest N(0, 0.3);
    m, v are a non-trivial optimizer state with v >= 0"""
    g_ = gen(seed)
    w = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_) * 0.3
    c = np.float32(ADAM_CLIP)
    up = np.nextafter(c, np.float32(1), dtype=np.float32)
    special = torch.tensor([c, -c, up, -up, 0.0, 1e-20, -1e-20], dtype=torch.float32)
    k = min(n, special.numel())
    g[:k] = (special if n >= special.numel() else special.roll(-seed))[:k]  # (n = 1: the seed picks which special value is met)
    m = torch.randn(n, generator=g_) * 0.05
    v = (torch.randn(n, generator=g_) * 0.05) ** 2
    return w, g, m, v


def adam_gradients(g0):
    """the gradients of two consecutive applies (the second: reversed and scaled, so that other elements meet the clip)"""
    return g0, g0.flip(0) * 1.5


def loss_case(B, H, W, mask_kind, seed, equal_pred=False):
    """flow [B,H,W,2], mask [B,H,W,1] ('zeros' / 'ones' / 'random'), pred3 [3B,H,W,2]; equal_pred: pred3[:B] == flow"""
    g = gen(seed)
    flow = torch.randn(B, H, W, 2, generator=g) * 0.3
    mask = {"zeros": torch.zeros(B, H, W, 1), "ones": torch.ones(B, H, W, 1), "random": torch.rand(B, H, W, 1, generator=g)}[mask_kind]
    pred3 = torch.randn(3 * B, H, W, 2, generator=g) * 0.3
    if equal_pred:
        pred3[:B] = flow
    return flow, mask, pred3


def flow_case(B, HW, seed):
    """flow [B, HW, 2] with its own mean and scale per sample and channel, |mean| <= 4 std"""
    g = gen(seed)
    scale = 0.05 + 3.0 * torch.rand(B, 1, 2, generator=g)
    mean = (torch.rand(B, 1, 2, generator=g) * 2 - 1) * 3.0 * scale
    z = torch.randn(B, HW, 2, generator=g)
    if HW > 1:
        z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True).clamp_min(1e-3)
    return (z * scale + mean).contiguous()


BHW_CASES = ((1, 1, 1), (1, 3, 5), (2, 1, 257), (1, 257, 1), (3, 7, 9), (2, 6, 12), (3, 33, 40))  # P = B H W: flat kernels see only P
EMIT_CASES = ((1, 4, 1, 2), (15, 8, 2, 3), (257, 12, 4, 8), (189, 5, 0, 5))  # (P, ld, coff, C)
ELU_ALPHA = 1.0
ADAM_N = (1, 255, 257, 2048 * 256 + 513)  # the last one: past the 2048-workgroup grid cap, the stride loop runs twice (and a tail)
ADAM_T = (1, 2, 1000, 100000)
LOSS_SHAPES = tuple((B, H, W) for B in (1, 3) for (H, W) in ((3, 5), (1, 257), (33, 40)))
LOSS_CBN = (0.5, 0.4, 1.0)
LOSS_MASKS = ("zeros", "ones", "random")
LOSS_EPS = (75.0, 1e-3)


def relmax(a, ref):
    """max |a - ref| relative to the largest |ref| (0 when both are all zero)"""
    d, s = float((a.double() - ref.double()).abs().max()), float(ref.double().abs().max())
    return d / s if s > 0 else (0.0 if d == 0 else float("inf"))


def measure_tolerances():
    """worst relmax of the float32 restatement against the float64 reference over the GPU tests' own inputs, per quantity"""
    worst = {k: 0.0 for k in TOL}

    def up(key, a, ref):
        worst[key] = max(worst[key], relmax(a, ref))

    for i, (B, H, W) in enumerate(BHW_CASES):
        P = B * H * W
        logits, f, dmask, dfin = mask_bwd_case(P, 40 + i)
        m32, fin32 = mask_composite_f32(logits[:, :2], f)
        m64, fin64 = mask_composite_f64(logits[:, :2], f)
        up("mask", m32, m64)
        up("fin", fin32, fin64)
        up("mask_bwd", mask_bwd_f32(m64.float(), f, dmask, dfin), mask_bwd_f64(logits[:, :2], f, dmask, dfin))
    for i, (P, ld, coff, C) in enumerate(EMIT_CASES):
        d, a = emit_case(P, ld, 60 + i)
        u0 = torch.zeros(P, ld)
        up("emit_elu", emit_du(d, a, coff, C, ACT_ELU, ELU_ALPHA, u0), emit_du(d.double(), a.double(), coff, C, ACT_ELU, ELU_ALPHA, u0))
    for i, n in enumerate(ADAM_N):
        for t in ADAM_T:
            w, g0, m, v = adam_case(n, 70 + i)
            s32, s64 = (w, m, v), (w.double(), m.double(), v.double())
            for k, g in enumerate(adam_gradients(g0)):  # two applies, each form carrying its own state, as the GPU test does
                gc = clip_f32(g, ADAM_CLIP)
                s32, s64 = adam_f32(s32[0], gc, s32[1], s32[2], t + k), adam_f64(s64[0], gc, s64[1], s64[2], t + k)
                up("adam_m", s32[1], s64[1])
                up("adam_v", s32[2], s64[2])
    for i, (B, H, W) in enumerate(LOSS_SHAPES):
        for cbn in LOSS_CBN:
            for kind in LOSS_MASKS:
                for eps in LOSS_EPS:
                    flow, mask, pred3 = loss_case(B, H, W, kind, 80 + i)
                    c32, c64 = coef_f32(flow, mask, pred3, cbn, eps), coef_f64(flow, mask, pred3, cbn, eps)
                    for j in range(4):  # each derivative against its own largest value
                        up("coef", c32[:, j], c64[:, j])
    return worst


# Tolerances that are measured, not picked: 4 x the worst deviation of the float32 restatement from the float64 reference over the GPU
# tests' own inputs (measure_tolerances; tests/test_glue_oracle.py::test_measured_tolerances re-measures and fails when a value here is
# not 4 x the measurement, or is above the cap of 1e-5).  All are relative to the largest reference value of the compared tensor.
TOL = {
    "mask": 4.31e-7,      # measured 1.077e-7 (mask_rec_inputs: the mask)
    "fin": 3.48e-7,       # measured 8.70e-8  (mask_rec_inputs: the recover inputs)
    "mask_bwd": 6.09e-7,  # measured 1.523e-7 (dlogits from the stored float32 mask)
    "emit_elu": 1.70e-7,  # measured 4.24e-8  (d * (a + 1))
    "adam_m": 8.15e-6,    # measured 2.039e-6 (two applies; the worst is n = 1, where m nearly cancels and float32(0.9) shows:
                          #                    1 - b1 is 0.100000024; over the long vectors it is 4e-7)
    "adam_v": 6.52e-7,    # measured 1.631e-7
    "coef": 1.50e-6,      # measured 3.74e-7  (each of the four derivatives against its own largest value)
}
TOL_CAP = 1e-5
