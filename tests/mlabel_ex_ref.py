"""CPU restatement, in numpy fp64, of the multi-label loss (mnasnet_pytorch_amd/losses.MultiLabelLoss, include/mnas.h "multi-label
loss"), written from the rule: the asymmetric focal loss with a margin, pos_weight, binary label smoothing and mixed label rows, with
its CLOSED-FORM gradient (the focusing weights differentiated).  `formula_torch` is the same loss as a differentiable fp64 torch
expression, for autograd to hold the closed form to.  Not a test: imported by test_mlabel_ex_cpu.py and the GPU tests."""
import numpy as np
import torch

# (gamma_pos, gamma_neg, margin, label_smoothing): plain, smoothed, symmetric focal, the ASL recipe, negative focusing with a
# margin, and a wide margin with gamma- = 1 (sigma_m^(gamma- - 1) = 1)
CONFIGS = ((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.1), (2.0, 2.0, 0.0, 0.0), (1.0, 4.0, 0.05, 0.1), (0.0, 4.0, 0.05, 0.0), (0.0, 1.0, 0.2, 0.0))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(z):
    ea = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + ea), ea / (1.0 + ea))


def mixed(Y, partner=None, lam=None):
    """the label matrix the loss sees before smoothing: lam Y + (1 - lam) Y[partner]"""
    Y = np.asarray(Y, dtype=np.float64)
    if partner is None:
        return Y
    lam = np.asarray(lam, dtype=np.float64)[:, None]
    return lam * Y + (1.0 - lam) * Y[np.asarray(partner)]


def dominant(Y, partner=None, lam=None):
    """the raw label rows the meters count: row n for lam >= 0.5, row partner_n otherwise"""
    Y = np.asarray(Y)
    if partner is None:
        return Y
    return np.where((np.asarray(lam) >= 0.5)[:, None], Y, Y[np.asarray(partner)])


def loss_and_grad(z, Y, w=None, pos_weight=None, gamma_pos=0.0, gamma_neg=0.0, margin=0.0, smoothing=0.0, reduction="mean",
                  partner=None, lam=None):
    """-> (loss, dloss/dz, e) in float64; e: the elements before the reduction"""
    z = np.asarray(z, dtype=np.float64)
    N, C = z.shape
    y = mixed(Y, partner, lam)
    t = (1.0 - smoothing) * y + smoothing / 2.0
    w = np.ones_like(z) if w is None else np.asarray(w, dtype=np.float64)
    p = np.ones(C) if pos_weight is None else np.asarray(pos_weight, dtype=np.float64)
    s = sigmoid(z)
    oms = sigmoid(-z)
    Lp = softplus(-z)
    Fp = np.exp(-gamma_pos * softplus(z))
    dpos = -Fp * (oms + gamma_pos * s * Lp)
    sm = np.maximum(s - margin, 0.0)
    live = s > margin                                    # strict
    with np.errstate(divide="ignore", invalid="ignore"):
        if margin == 0.0:
            Fn = np.exp(-gamma_neg * softplus(-z))
            Ln = softplus(z)
            dneg = Fn * (gamma_neg * oms * softplus(z) + s)
        else:
            lsm = np.log(np.where(live, sm, 1.0))
            Fn = np.where(live, np.exp(gamma_neg * lsm), 1.0 if gamma_neg == 0.0 else 0.0)
            Ln = np.where(live, -np.log1p(-sm), 0.0)
            pm1 = gamma_neg * np.exp((gamma_neg - 1.0) * lsm) if gamma_neg != 0.0 else np.zeros_like(z)
            dneg = np.where(live, s * oms * (pm1 * Ln + Fn / (1.0 - sm)), 0.0)
    e = w * (p * t * Fp * Lp + (1.0 - t) * Fn * Ln)
    D = float(N * C) if reduction == "mean" else float(N)
    g = w * (p * t * dpos + (1.0 - t) * dneg) / D
    return float(e.sum() / D), g, e


def formula_torch(z, Y, w=None, pos_weight=None, gamma_pos=0.0, gamma_neg=0.0, margin=0.0, smoothing=0.0, reduction="mean",
                  partner=None, lam=None):
    """the same loss, literally as the issue's formula, on fp64 torch tensors (z may require grad) -> 0-d tensor"""
    F = torch.nn.functional
    N, C = z.shape
    y = Y
    if partner is not None:
        y = lam[:, None] * Y + (1.0 - lam[:, None]) * Y[partner]
    t = (1.0 - smoothing) * y + smoothing / 2.0
    p = torch.ones(C, dtype=z.dtype) if pos_weight is None else pos_weight
    s = torch.sigmoid(z)
    Lp = F.softplus(-z)                                  # -log(sigma)
    Fp = torch.exp(-gamma_pos * F.softplus(z))           # (1 - sigma)^gamma+
    sm = (s - margin).clamp_min(0.0)
    Fn = sm ** gamma_neg                                 # (0^0 = 1)
    Ln = -torch.log1p(-sm)
    e = p * t * Fp * Lp + (1.0 - t) * Fn * Ln
    if w is not None:
        e = e * w
    return e.sum() / (N * C if reduction == "mean" else N)


def batch(N, C, seed=0, scale=2.0, density=0.3, soft=False):
    """(z, Y, w, pos_weight, partner, lam) fp32 torch tensors on the CPU: logits leaning towards the labels, weights in [0.25, 1.75),
    pos_weight in [0.5, 4.5), a random partner per row, lam from {0, 1, 0.5} and uniform values in turn"""
    g = torch.Generator().manual_seed(seed * 7919 + N * 1000 + C)
    Y = (torch.rand(N, C, generator=g) < density).float()
    if soft:
        Y = torch.tensor([0.0, 0.3, 1.0, 0.7])[torch.randint(0, 4, (N, C), generator=g)]
    z = (torch.randn(N, C, generator=g) + 0.8 * (2.0 * (Y > 0.5).float() - 1.0)) * scale
    w = 0.25 + 1.5 * torch.rand(N, C, generator=g)
    pw = 0.5 + 4.0 * torch.rand(C, generator=g)
    partner = torch.randint(0, N, (N,), generator=g)
    lam = torch.rand(N, generator=g)
    for k, v in enumerate((0.0, 1.0, 0.5)):
        if k < N:
            lam[k] = v
    return z, Y, w, pw, partner, lam
