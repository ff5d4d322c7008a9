"""CPU restatement, in fp64, of the distillation cross-entropy (mnasnet_pytorch_amd/losses.DistillCrossEntropyLoss, include/mnas.h
"distillation cross-entropy"), written from the rule and with its closed-form gradient.  tests/test_kd_cpu.py holds it to torch's own
composition -- F.cross_entropy(weight=, label_smoothing=) plus T^2 kl_div(batchmean) -- and to autograd; the GPU tests compare the
kernels with it."""
import torch


def kd_loss(z, a, b=None, lam=None, eps=0.0, w=None, t=None, T=1.0, alpha=0.5, ignore_index=-100):
    """z (N, C) logits; a (and b, lam: a mixed batch) the labels; w (C,) class weights or None; t (N, C) teacher logits or None.
        q_n    = (1 - eps) (lam e[a] + (1 - lam) e[b]) + eps / C
        hard_n = -sum_c w_c q_nc log softmax(z_n)_c          (0 for a row with an ignored label; a class with q_nc == 0 adds 0)
        D      = sum over the rows not ignored of lam w[a] + (1 - lam) w[b],   hard = sum_n hard_n / D
        kd_n   = sum_c pT_c (log pT_c - log pS_c),  pT = softmax(t_n / T), pS = softmax(z_n / T)   (a class with pT_c == 0 adds 0)
        kd     = T^2 sum_n kd_n / N over ALL rows
        loss   = (1 - alpha) hard + alpha kd;  hard alone when t is None or alpha == 0;  kd alone when alpha == 1
    Gradient: (1 - alpha) (p S_n - w q_n) / D + alpha T (pS - pT) / N with S_n = sum_c w_c q_nc.
    -> dict(loss, hard, kd, grad, hard_rows, kd_rows, D) in fp64."""
    z = z.detach().double()
    N, C = z.shape
    b = a if b is None else b
    lam = torch.ones(N, dtype=torch.float64) if lam is None else lam.double()
    w = torch.ones(C, dtype=torch.float64) if w is None else w.double()
    keep = (a != ignore_index) & (b != ignore_index)
    a0, b0 = torch.where(keep, a, torch.zeros_like(a)), torch.where(keep, b, torch.zeros_like(b))
    rows = torch.arange(N)
    q = torch.zeros(N, C, dtype=torch.float64)
    q[rows, a0] += (1.0 - eps) * lam
    q[rows, b0] += (1.0 - eps) * (1.0 - lam)
    q = q + eps / C
    logp = torch.log_softmax(z, 1)
    wq = w[None, :] * q
    hard_rows = -torch.where(q == 0, torch.zeros_like(q), wq * logp).sum(1)
    hard_rows = torch.where(keep, hard_rows, torch.zeros_like(hard_rows))
    s = lam * w[a0] + (1.0 - lam) * w[b0]
    D = (s * keep).sum()
    hard = hard_rows.sum() / D if float(D) != 0.0 else torch.tensor(float("nan"), dtype=torch.float64)
    ghard = torch.zeros_like(z)
    if float(D) != 0.0:
        ghard = (torch.exp(logp) * wq.sum(1, keepdim=True) - wq) / D * keep[:, None]
    use_kd = t is not None and alpha != 0.0
    kd_rows, kd, gkd = torch.zeros(N, dtype=torch.float64), torch.zeros((), dtype=torch.float64), torch.zeros_like(z)
    if use_kd:
        lpT, lpS = torch.log_softmax(t.detach().double() / T, 1), torch.log_softmax(z / T, 1)
        pT = torch.exp(lpT)
        kd_rows = torch.where(pT > 0, pT * (lpT - lpS), torch.zeros_like(pT)).sum(1)
        kd = T * T * kd_rows.sum() / N
        gkd = T * (torch.exp(lpS) - pT) / N
    if not use_kd:
        loss, grad = hard, ghard
    elif alpha == 1.0:
        loss, grad = kd, gkd
    else:
        loss, grad = (1.0 - alpha) * hard + alpha * kd, (1.0 - alpha) * ghard + alpha * gkd
    return dict(loss=loss, hard=hard, kd=kd, grad=grad, hard_rows=hard_rows, kd_rows=kd_rows, D=D)
