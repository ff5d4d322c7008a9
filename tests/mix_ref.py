"""CPU restatement of batch mixing and of the soft-target cross-entropy (mnasnet_pytorch_amd/mixing.py, losses.MixCrossEntropyLoss,
include/mnas.h "soft-target cross-entropy" / "batch mixing"), written from the rule: the loss from F.cross_entropy in fp64, the
byte arithmetic in numpy integers, the draws from the documented order.  tests/test_mix_cpu.py holds the closed form and the draw
order to it; the GPU tests compare the kernels with it."""
import math
import random

import numpy as np
import torch
import torch.nn.functional as F

NONE, MIXUP, CUTMIX = 0, 1, 2


# ---- loss -------------------------------------------------------------------------------------------------------------------------
def soft_ce(z, a, b=None, lam=None, eps=0.0, ignore_index=-100):
    """The oracle: per row lam CE(a) + (1 - lam) CE(b) with CE = F.cross_entropy(label_smoothing=eps, reduction='none') in fp64,
    rows with an ignored label dropped, mean over the rest.  -> (loss 0-d fp64, dloss/dz fp64 (N, C)); every row ignored: NaN."""
    z = z.detach().double().clone().requires_grad_(True)
    N = z.shape[0]
    b = a if b is None else b
    lam = torch.ones(N, dtype=torch.float64) if lam is None else lam.double()
    keep = (a != ignore_index) & (b != ignore_index)
    a0, b0 = torch.where(keep, a, torch.zeros_like(a)), torch.where(keep, b, torch.zeros_like(b))
    rows = lam * F.cross_entropy(z, a0, label_smoothing=eps, reduction="none") + \
        (1.0 - lam) * F.cross_entropy(z, b0, label_smoothing=eps, reduction="none")
    count = int(keep.sum())
    if count == 0:
        return torch.tensor(float("nan"), dtype=torch.float64), torch.zeros_like(z).detach()
    loss = (rows * keep).sum() / count
    loss.backward()
    return loss.detach(), z.grad


def soft_ce_closed_form(z, a, b=None, lam=None, eps=0.0, ignore_index=-100):
    """The kernel's formulas in fp64: row = (1 - eps) (lam (lse - z[a]) + (1 - lam) (lse - z[b])) + eps (lse - mean z),
    dlogits = (softmax - q) / count, q = (1 - eps) (lam e[a] + (1 - lam) e[b]) + eps / C"""
    z = z.double()
    N, C = z.shape
    b = a if b is None else b
    lam = torch.ones(N, dtype=torch.float64) if lam is None else lam.double()
    keep = (a != ignore_index) & (b != ignore_index)
    count = int(keep.sum())
    lse = torch.logsumexp(z, 1)
    loss, grad = 0.0, torch.zeros_like(z)
    for n in range(N):
        if not keep[n]:
            continue
        la, lb = float(lam[n]), 1.0 - float(lam[n])
        loss = loss + (1 - eps) * (la * (lse[n] - z[n, a[n]]) + lb * (lse[n] - z[n, b[n]])) + eps * (lse[n] - z[n].mean())
        q = torch.full((C,), eps / C, dtype=torch.float64)
        q[a[n]] += (1 - eps) * la
        q[b[n]] += (1 - eps) * lb
        grad[n] = (torch.softmax(z[n], 0) - q) / count
    if count == 0:
        return torch.tensor(float("nan"), dtype=torch.float64), grad
    return loss / count, grad


def dominant(a, b, lam):
    """the label a row is ranked against: a when lam >= 0.5"""
    return torch.where(lam >= 0.5, a, b)


# ---- bytes ------------------------------------------------------------------------------------------------------------------------
def blend(x, p, w16):
    """(w x + (65536 - w) p + 32768) >> 16 per byte, in 64-bit integers"""
    x, p = np.asarray(x).astype(np.int64), np.asarray(p).astype(np.int64)
    return ((w16 * x + (65536 - w16) * p + 32768) >> 16).astype(np.uint8)


def mix_one(x, p, mode, w16=65536, box=(0, 0, 0, 0)):
    """one (3, H, W) image against its partner"""
    if mode == NONE:
        return x.copy()
    if mode == MIXUP:
        return blend(x, p, w16)
    y0, x0, y1, x1 = box
    out = x.copy()
    out[:, y0:y1, x0:x1] = p[:, y0:y1, x0:x1]
    return out


def mix_batch(x, draws):
    """x: (n, 3, H, W) uint8; draws: (mode, partner, w16, box, ...) per image -> the mixed batch, every partner read from x"""
    return np.stack([mix_one(x[k], x[d[1]], d[0], d[2], d[3]) for k, d in enumerate(draws)])


# ---- draws ------------------------------------------------------------------------------------------------------------------------
def box_of(h, w, lam, cy, cx):
    """the CutMix paper's box and the weight the pixels really get"""
    r = math.sqrt(1.0 - lam)
    ch, cw = int(h * r), int(w * r)
    y0, y1 = int(np.clip(cy - ch // 2, 0, h)), int(np.clip(cy + ch // 2, 0, h))
    x0, x1 = int(np.clip(cx - cw // 2, 0, w)), int(np.clip(cx + cw // 2, 0, w))
    return (y0, x0, y1, x1), 1.0 - (y1 - y0) * (x1 - x0) / float(h * w)


def describe(n, h, w, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, per_sample=False):
    """DeviceMix.describe from its documented draw order -> [(mode, partner, w16, box, lam)]"""
    if n == 0:
        return []
    partners = random.sample(range(n), n)

    def one():
        u = random.random()
        if not (u < prob and (mixup_alpha > 0 or cutmix_alpha > 0)):
            return (NONE, 65536, (0, 0, 0, 0), 1.0)
        if mixup_alpha > 0 and cutmix_alpha > 0:
            cut = random.random() < switch_prob
        else:
            cut = cutmix_alpha > 0
        if cut:
            lam = random.betavariate(cutmix_alpha, cutmix_alpha)
            cy = random.randrange(h)
            cx = random.randrange(w)
            box, eff = box_of(h, w, lam, cy, cx)
            return (CUTMIX, 65536, box, eff)
        lam = random.betavariate(mixup_alpha, mixup_alpha)
        w16 = int(round(lam * 65536.0))
        return (MIXUP, w16, (0, 0, 0, 0), w16 / 65536.0)

    draws = [one() for _ in range(n)] if per_sample else [one()] * n
    return [(m, k if m == NONE else partners[k], w16, box, lam) for k, (m, w16, box, lam) in enumerate(draws)]
