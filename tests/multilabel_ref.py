"""CPU restatement of the multi-label branch (mnasnet_pytorch_amd/losses.py, metrics.MultiLabelMeters, include/mnas.h
"MnasMultiLabelMeters"), written from the rule, not from the reference's text: the BCE-with-logits loss with optional element weights
and the focal transform of the MEAN, its gradient, the per-row macro-F1 over the labels present, HardDice, and the AverageMeter
arithmetic in Python floats.  tests/golden/multilabel.json holds what the reference's own MultiClassBCELoss / HardDice / batch_metrics
gave on the same inputs; test_multilabel_cpu.py holds this file to it."""
import numpy as np
import torch

from metrics_ref import Meter  # noqa: F401  (the AverageMeter arithmetic is the same for every meter)

GRID_C = (5, 90, 1000)
GRID_SCALE = (0.5, 2.0, 8.0)
GRID_DENSITY = (0.02, 0.3)
GRID_SEEDS = tuple(range(5))
GRID_N = 12
FOCUS, BALANCE = 2, 0.25                 # the reference's defaults
LOSS_VARIANTS = (("plain", False, False), ("weighted", True, False), ("focal", False, True), ("weighted_focal", True, True))


def grid_batch(C, scale, density, seed, N=GRID_N):
    """One batch of the fixture's input grid: (logits, target, weights), fp32 [N][C].  The logits lean towards the labels (a true class
    is shifted up by 0.8 scale, a false one down), so every count of the metrics is exercised; weights in [0.25, 1.75)."""
    g = torch.Generator().manual_seed(seed * 1000 + C)
    t = (torch.rand(N, C, generator=g) < density).float()
    z = (torch.randn(N, C, generator=g) + 0.8 * (2.0 * t - 1.0)) * scale
    w = 0.25 + 1.5 * torch.rand(N, C, generator=g)
    return z, t, w


def grid():
    for C in GRID_C:
        for scale in GRID_SCALE:
            for density in GRID_DENSITY:
                for seed in GRID_SEEDS:
                    yield C, scale, density, seed


def grid_key(C, scale, density, seed):
    return "C%d_s%g_d%g_seed%d" % (C, scale, density, seed)


# ---- loss ---------------------------------------------------------------------------------------------------------------
def bce(z, t, w=None, focal=False, focus_param=FOCUS, balance_param=BALANCE):
    """-> (loss, dloss/dz) in float64: e = max(z,0) - z t + log1p(exp(-|z|)) (times w), b = mean(e); focal: pt = exp(-b),
    loss = balance (1-pt)^gamma b, applied to the mean"""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    w = np.ones_like(z) if w is None else np.asarray(w, dtype=np.float64)
    ea = np.exp(-np.abs(z))
    e = (np.maximum(z, 0.0) - z * t + np.log1p(ea)) * w
    b = e.sum() / z.size
    sig = np.where(z >= 0, 1.0 / (1.0 + ea), ea / (1.0 + ea))
    g = w * (sig - t) / z.size
    if not focal:
        return float(b), g
    pt = np.exp(-b)
    loss = balance_param * (1.0 - pt) ** focus_param * b
    s = balance_param * (1.0 - pt) ** (focus_param - 1) * ((1.0 - pt) + focus_param * pt * b)
    return float(loss), s * g


# ---- metrics ------------------------------------------------------------------------------------------------------------
def f1_rows(z, t):
    """per row: predicted iff z >= 0, true iff t == 1; mean of F1_1 = 2tp/(2tp+fp+fn) (if tp+fp+fn > 0) and F1_0 = 2tn/(2tn+fp+fn)
    (if tn+fp+fn > 0) -- the macro average over the labels that occur in the row.  Python floats."""
    z = np.asarray(z, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    out = []
    for zr, tr in zip(z, t):
        p, y = zr >= 0, tr == 1
        tp, fp, fn, tn = int((p & y).sum()), int((p & ~y).sum()), int((~p & y).sum()), int((~p & ~y).sum())
        fs = []
        if tp + fp + fn > 0:
            fs.append(2 * tp / (2 * tp + fp + fn))
        if tn + fp + fn > 0:
            fs.append(2 * tn / (2 * tn + fp + fn))
        out.append(fs[0] if len(fs) == 1 else (fs[0] + fs[1]) / 2)
    return out


def f1_batch(z, t):
    """(sum of the rows' F1 in row order, one rounded double sum per row) / N"""
    s = 0.0
    rows = f1_rows(z, t)
    for f in rows:
        s = s + f
    return s / len(rows)


def dice_counts(z, t, threshold_logit=0.0):
    """(tp, fp, fn) under the Dice rule: predicted iff z > threshold_logit (strict)"""
    z = np.asarray(z, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    p, y = z > np.float32(threshold_logit), t == 1
    return int((p & y).sum()), int((p & ~y).sum()), int((~p & y).sum())


def hard_dice(z, t, threshold_logit=0.0, deduct_intersection=False):
    """clamp(1 + log(2I/U), 0, 1) in fp32; 0 when I == 0"""
    tp, fp, fn = dice_counts(z, t, threshold_logit)
    if tp == 0:
        return 0.0
    U = (tp + fp) + (tp + fn) - (tp if deduct_intersection else 0)
    v = np.float32(1) + np.log(np.float32(2 * tp) / np.float32(U), dtype=np.float32)
    return float(min(max(v, np.float32(0)), np.float32(1)))


def meter_inputs(updates=10):
    """(loss values, dice values, f1 values, n_loss_and_dice, n_f1) of the fixture's AverageMeter trace: the first `updates` batches of
    the C = 90 part of the grid (fp32 losses and Dice read back as Python floats), unequal batch sizes for the first two meters and
    the number of classes for the third (train.py:463)"""
    losses, dices, f1s = [], [], []
    for (C, scale, density, seed) in [c for c in grid() if c[0] == 90][:updates]:
        z, t, _ = grid_batch(C, scale, density, seed)
        losses.append(float(np.float32(bce(z.numpy(), t.numpy())[0])))
        dices.append(hard_dice(z.numpy(), t.numpy()))
        f1s.append(f1_batch(z.numpy(), t.numpy()))
    ns = [256] * (updates - 1) + [100]
    return losses, dices, f1s, ns, [90] * updates


class StepLog:
    """What a MultiLabelMeters block must hold after a sequence of updates fed with the DEVICE's own per-batch values"""

    def __init__(self):
        self.loss, self.hdice, self.f1 = Meter(), Meter(), Meter()
        self.tp = self.fp = self.fn = self.steps = self.samples = self.nonfinite = 0
        self.last = (0, 0, 0)

    def update(self, z, t, loss, dice, f1, n_loss, n_dice, n_f1):
        c = dice_counts(z, t)
        self.tp, self.fp, self.fn = self.tp + c[0], self.fp + c[1], self.fn + c[2]
        self.last = c
        self.steps += 1
        self.samples += int(np.asarray(z).shape[0])
        self.hdice.update(dice, n_dice)
        self.f1.update(f1, n_f1)
        if loss is not None:
            self.loss.update(loss, n_loss)
            if not np.isfinite(loss):
                self.nonfinite += 1

    def check(self, rec):
        """rec: metrics.MultiLabelRecord -- everything exactly"""
        assert (rec.steps, rec.samples, rec.nonfinite_steps) == (self.steps, self.samples, self.nonfinite)
        assert (rec.tp, rec.fp, rec.fn) == (self.tp, self.fp, self.fn)
        assert (rec.last_tp, rec.last_fp, rec.last_fn) == self.last
        same = lambda a, b: a == b or (a != a and b != b)     # noqa: E731  (NaN equals NaN here)
        for name, m in (("loss", self.loss), ("hdice", self.hdice), ("f1", self.f1)):
            if not m.count:
                continue
            got = getattr(rec, name)
            assert same(got.val, m.val) and same(got.avg, m.avg), (name, got, m.state())
            assert same(getattr(rec, name + "_sum"), m.sum) and getattr(rec, name + "_n") == m.count, (name, m.state())
