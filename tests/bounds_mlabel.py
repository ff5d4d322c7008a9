"""Per-element bounds for the multi-label loss (csrc/mnas_mlabel.hip: k_mlabel_row, k_mlabel_batch, k_mlabel_scale) and HardDice.
Conventions of intervals.py.  mnas_mlabel.o is built with -ffp-contract=on: a multiply may fuse with the add of the SAME expression,
so `- z*t +` and `ls += e*w` are bracketed as the hull of their fused and unfused forms.  expf, log1pf, logf and the divisions are
taken at ONE ULP (2u relative; a subnormal result: 2^-149 absolute), the assumption ce_intervals makes."""
import math

import torch

from intervals import D64, TINY32, Interval, f32, round32, widen, widen64

exact = Interval.exact
ULP1 = dict(n=1, ulps=2, floor=True, host=D64)     # a one-ulp fp32 function of a value known to lie between two fp64 results


def _mul64(a, b, n=1):
    p = a.mul(b, 0)
    return Interval(*widen64(p.lo, p.hi, n))


ML_SHAPES = [(1, 1), (3, 5), (5, 257), (2, 1000), (3, 1024), (3, 1028), (2, 2052), (3, 1027), (257, 3), (513, 4)]
ML_KINDS = ["scale0.5", "scale8", "scale30", "edges", "confident", "soft", "pow2w", "sparse"]
ML_EDGE_Z = [0.0, -0.0, 17.0, -17.0, 18.0, -18.0, 88.0, -88.0, 90.0, -90.0, 104.0, -104.0, 200.0, -200.0]
ML_LIVE_COLS = (0, 255, 256, 1023, 1024)
ML_FOCAL = ((1.0, 0.25), (2.0, 0.25), (3.5, 0.75))          # (focus_param, balance_param) of the focal cases
ML_BIG = (1100, 1000)                                       # N*C > 4096*256: k_mlabel_scale's grid-stride second trip


def mlabel_live(N, C_):
    """the sparse probe's live element of every row: columns 0, 255, 256, 1023, 1024 and C-1 (those that exist) in turn"""
    cols = sorted({c for c in ML_LIVE_COLS + (C_ - 1,) if c < C_})
    return [(n, cols[n % len(cols)]) for n in range(N)]


def mlabel_inputs(kind, N, C_):
    """(z, t, w) fp32 [N][C] of the multi-label bound tests (CPU proofs and GPU cases read the same).  scale*: logits leaning
    towards the labels times 0.5 / 8 / 30; edges: z through +-0 and |z| = 17, 18 (ea below 2^-24), 88, 90 (ea subnormal), 104, 200
    (ea zero), against both targets; confident: z = +-(18..30) agreeing with t everywhere (log1pf(ea) is the whole loss); soft:
    targets 0, 0.3, 0.7, 1; pow2w: weights 2^-12..2^12 and exact zeros; sparse: ONE live weight per row (mlabel_live)."""
    g = torch.Generator().manual_seed(N * 1000 + C_ + 7)
    t = (torch.rand(N, C_, generator=g) < 0.4).float()
    u = torch.randn(N, C_, generator=g)
    w = 0.25 + 1.5 * torch.rand(N, C_, generator=g)
    if kind.startswith("scale"):
        return (u + 0.5 * (2 * t - 1)) * float(kind[5:]), t, w
    if kind == "edges":
        i = torch.arange(N * C_)
        z = torch.tensor(ML_EDGE_Z)[i % len(ML_EDGE_Z)].view(N, C_)
        return z, ((i // len(ML_EDGE_Z)) % 2).float().view(N, C_), w
    if kind == "confident":
        return (2 * t - 1) * (18.0 + 12.0 * torch.rand(N, C_, generator=g)), t, w
    z = (u + 0.5 * (2 * t - 1)) * 2.0
    if kind == "soft":
        return z, torch.tensor([0.0, 0.3, 1.0, 0.7])[torch.randint(0, 4, (N, C_), generator=g)], w
    if kind == "pow2w":
        w = torch.pow(torch.tensor(2.0), torch.randint(-12, 13, (N, C_), generator=g).float())
        w[torch.rand(N, C_, generator=g) < 0.2] = 0.0
        return z, t, w
    assert kind == "sparse"
    w = torch.zeros(N, C_)
    for (n, c) in mlabel_live(N, C_):
        w[n, c] = 1.0
    return z, t, w


def mlabel_inv(N, C_):
    """r.inv of mnas_mlabel_bce, bit for bit: (float)(1.0 / ((double)N * (double)C))"""
    return float(torch.tensor(1.0 / (float(N) * float(C_)), dtype=torch.float64).float())


def mlabel_trips(C_, vec):
    """terms a lane of k_mlabel_row adds: ceil(C/256) on the scalar path, 4 ceil(C/1024) on the vector path"""
    return 4 * -(-C_ // 1024) if vec else -(-C_ // 256)


def mlabel_batch_intervals(rows_dev, N, C_, focal, gamma, balance):
    """k_mlabel_batch's loss (and, focal, the gradient's factor s) from the loss_rows the device stored (exact data): the double
    sum in a fixed order (relative D64 = 2^-48 of sum|rows|, all of it the device's: the host's centre is math.fsum's correctly
    rounded sum), one double division by N*C, ONE rounding to fp32: b.  Focal, all in
    double, operation by operation at one double ulp each (two where the host's own exp / pow is in the chain): pt = exp(-b),
    om = 1 - pt, loss = (float)((balance * pow(om, g)) * b), s = (float)((balance * pow(om, g - 1)) * (om + (g * pt) * b)).  om
    cancels for a tiny b: it is then known to 2^-52 / b relative only, and so are the loss and s -- the kernel's own operation.
    gamma, balance: the fp32 values the ABI passes.  -> dict(b=, loss=, s= (None without focal)) of 0-dim Intervals."""
    r = rows_dev.detach().cpu().double().reshape(-1)                 # (N numbers: on the host, whichever device the rest runs on)
    S = torch.tensor(math.fsum(r.tolist()), dtype=torch.float64)    # (the bracket's centre: the correctly rounded sum, so that D64
    Sa = torch.tensor(math.fsum(r.abs().tolist()), dtype=torch.float64)   # is the device's allowance alone)
    den = float(N) * float(C_)
    lo, hi = (S - D64 * Sa) / den, (S + D64 * Sa) / den
    lo, hi = widen64(lo, hi, 1)
    b = Interval(round32(lo), round32(hi))
    if not focal:
        return dict(b=b, loss=b, s=None)
    g, bal = exact(f32(gamma), like=r), exact(f32(balance), like=r)
    pt = Interval(*widen64(torch.exp(-b.hi), torch.exp(-b.lo), 2))
    olo, ohi = widen64(1.0 - pt.hi, 1.0 - pt.lo, 1)
    om = Interval(olo.clamp_min(0.0), ohi.clamp_min(0.0))
    pw = Interval(*widen64(torch.pow(om.lo, g.lo), torch.pow(om.hi, g.lo), 2))
    pw1 = Interval(*widen64(torch.pow(om.lo, g.lo - 1.0), torch.pow(om.hi, g.lo - 1.0), 2))
    loss = _mul64(_mul64(bal, pw), b)
    gp = _mul64(_mul64(g, pt), b)
    inner = Interval(*widen64(om.lo + gp.lo, om.hi + gp.hi, 1))
    s = _mul64(_mul64(bal, pw1), inner)
    return dict(b=b, loss=Interval(round32(loss.lo), round32(loss.hi)), s=Interval(round32(s.lo), round32(s.hi)))


def mlabel_intervals(z, t, w, N, C_, focal, gamma, balance, vec, rows_dev=None):
    """Brackets of every output of mnas_mlabel_bce, by interval propagation through ml_elem as written; z, t, w (None: no weights)
    fp32 [N][C] as the device reads them, on any device (the fp64 work runs where z lives).
      ea = expf(-|z|) and log1pf(ea) at one ulp; m = fmaxf(z, 0) exact; A = m - z*t: fl(m - z t) fused, fl(m - fl(z t)) unfused,
      the hull; e = fl(A + log1pf(ea)); the row's term e*w: exact inside a fused ls += e*w, fl(e w) unfused, the hull (w NULL: e).
      sg: z >= 0 (-0.0 too): 1/fl(1 + ea); z < 0: ea/fl(1 + ea) -- each branch bracketed on its own elements, division one ulp;
      dlogits = fl(fl(w fl(sg - t)) inv), inv = mlabel_inv(N, C) (no multiply feeds an add there: nothing to fuse).  sg - t
      cancels for a confident true class; that is the kernel's arithmetic and the bracket follows it.
      row sums: a lane adds T = mlabel_trips(C, vec) terms, then 6 butterfly adds and 3 adds of the four waves:
          |row - sum mid(e w)| <= (T + 9) 2^-23 sum|e w| + sum half(e w)        (check_sum_bound's form; no term excluded).
    rows_dev (the device's loss_rows, scratch byte 8 N): adds mlabel_batch_intervals' b, loss and s; focal: dlogits is the unscaled
    bracket times the bracket of s, one rounding more (k_mlabel_scale).
    -> dict(dl, dl_unscaled, ew, rows, row_half, [b, loss, s])."""
    z, t = z.double(), t.double()
    one = exact(1.0, like=z)
    a = z.abs()
    elo, ehi = widen(torch.exp(-a), torch.exp(-a), **ULP1)
    ea = Interval(elo.clamp_min(0.0), ehi)
    llo, lhi = widen(torch.log1p(ea.lo), torch.log1p(ea.hi), **ULP1)
    l1 = Interval(llo.clamp_min(0.0), lhi)
    m, zt = z.clamp_min(0.0), z * t                                   # (fp32 x fp32: exact in double)
    fl_, fh = widen(m - zt, m - zt, 1, floor=True)
    zr = round32(zt)                                                  # (the unfused product: ONE known fp32 number)
    ul, uh = widen(m - zr, m - zr, 1, floor=True)
    A = Interval(torch.minimum(fl_, ul), torch.maximum(fh, uh))
    e = A.add(l1, 1)
    if w is None:
        ew, wv = e, None
    else:
        wv = exact(w.double())
        ex, un = e.mul(wv, 0), e.mul(wv, 1)
        ew = Interval(torch.minimum(ex.lo, un.lo - TINY32), torch.maximum(ex.hi, un.hi + TINY32))
    T = mlabel_trips(C_, vec)
    row_half = (T + 9) * 2.0 ** -23 * ew.amax.sum(1) + ew.half.sum(1)
    rows = Interval(ew.mid.sum(1) - row_half, ew.mid.sum(1) + row_half)
    d = one.add(ea, 1)
    sp, sn = one.div(d, 1, 2), ea.div(d, 1, 2)
    pos = z >= 0
    sg = Interval(torch.where(pos, sp.lo, sn.lo), torch.where(pos, sp.hi, sn.hi))
    df = sg.add(exact(t), 1, -1.0)
    if wv is not None:
        df = wv.mul(df, 1)
    dl0 = df.mul(exact(mlabel_inv(N, C_), like=z), 1)
    dl0 = Interval(dl0.lo - TINY32, dl0.hi + TINY32)
    out = dict(dl=dl0, dl_unscaled=dl0, ew=ew, rows=rows, row_half=row_half)
    if rows_dev is not None:
        out.update(mlabel_batch_intervals(rows_dev, N, C_, focal, gamma, balance))
        if focal:
            s = out["s"]
            sc = dl0.mul(Interval(s.lo.to(z.device), s.hi.to(z.device)), 1)
            out["dl"] = Interval(sc.lo - TINY32, sc.hi + TINY32)
    elif focal:
        out["dl"] = None
    return out


def mlabel_probe_visible(iv, live, what):
    """the sparse probe of the multi-label rows: every live element's loss term (lower end) exceeds twice its row's bound"""
    lo = iv["ew"].lo
    for (n, c) in live:
        assert float(lo[n, c]) > 2 * float(iv["row_half"][n]), "%s: the live term (%d, %d) would not be seen" % (what, n, c)


def dice_interval(I, P, T, deduct):
    """ml_dice: 0 when I <= 0; else U = P + T - (deduct ? I : 0), a = (float)(2 I), b = (float)U each rounded as the int64 ->
    fp32 conversion rounds (to nearest even; exact below 2^24), q = a / b and logf(q) at one ulp, v = fl(1 + logf(q)), the clamp
    to [0, 1] applied to both ends.  -> 0-dim Interval."""
    if I <= 0:
        return exact(0.0)
    U = P + T - (I if deduct else 0)
    a, b = round32(torch.tensor(float(2 * I), dtype=torch.float64)), round32(torch.tensor(float(U), dtype=torch.float64))
    q = Interval(a, a).div(Interval(b, b), 1, 2)
    lg = Interval(*widen(torch.log(q.lo), torch.log(q.hi), **ULP1))
    v = exact(1.0).add(lg, 1)
    return Interval(v.lo.clamp(0.0, 1.0), v.hi.clamp(0.0, 1.0))
