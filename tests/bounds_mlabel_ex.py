"""Per-element bounds for mnas_mlabel_loss (csrc/mnas_mlabel.hip: k_mlabel_row_ex, k_mlabel_batch), on intervals.py with
bounds_mlabel.py's conventions: expf, logf, log1pf and the divisions are taken at ONE ULP (2u relative; a subnormal result: 2^-149
absolute), every other operation is correctly rounded.  mnas_mlabel.o is built with -ffp-contract=on.  The general element
(mlx_asym) writes each multiply that feeds an add as an explicit fmaf and everything else as a statement of its own, so its
roundings are the ones in the source and the bracket follows them one by one.  The plain element is ml_bce, whose `- z*t +` and
`ls += e*w` may or may not fuse: those are the hull of both forms, as in bounds_mlabel.mlabel_intervals -- here with t itself an
interval, because mixing and smoothing round.  Nothing is fitted to a kernel's output.

The margin's hinge: sigma_m = fl(sigma - m) > 0 decides the negative branch on the DEVICE's sigma.  Where the bracket of sigma_m
contains 0 the device may take either side, and the bracket is the hull of both (for gamma- = 0 the gradient jumps there, by the
rule itself)."""
import math

import torch

from bounds_mlabel import ULP1, mlabel_trips
from intervals import D64, TINY32, Interval, f32, round32, widen, widen64

exact = Interval.exact

# (gamma_pos, gamma_neg, margin, smoothing, pos_weight?) of the GPU cases
EX_CONFIGS = ((0.0, 0.0, 0.0, 0.0, True), (2.0, 2.0, 0.0, 0.0, False), (1.0, 4.0, 0.05, 0.1, True), (0.0, 4.0, 0.05, 0.0, False))
EX_SHAPES = [(1, 1), (3, 5), (7, 63), (7, 65), (5, 257), (2, 1000), (3, 1024), (2, 2052), (257, 3)]


def _f1(fn, iv, clamp0=False):
    """a one-ulp fp32 function, increasing, of a value inside iv"""
    lo, hi = widen(fn(iv.lo), fn(iv.hi), **ULP1)
    return Interval(lo.clamp_min(0.0) if clamp0 else lo, hi)


def _neg(iv):
    return Interval(-iv.hi, -iv.lo)


def _hull(a, b):
    return Interval(torch.minimum(a.lo, b.lo), torch.maximum(a.hi, b.hi))


def _where(mask, a, b):
    return Interval(torch.where(mask, a.lo, b.lo), torch.where(mask, a.hi, b.hi))


def _full(v, like):
    return exact(torch.full_like(like, v))


def label_intervals(Y, partner, lam, smoothing):
    """t as the kernel forms it from the raw fp32 labels Y [N][C]: mixed rows y = fma(lam, Y, fl(fl(1 - lam) * Y[partner])), then
    smoothing t = fma(fl(1 - eps), y, eps/2) with eps the fp32 value the ABI passes (eps/2 is exact).  partner / lam None: no mixing;
    smoothing 0: no operation."""
    y = exact(Y.double())
    if partner is not None:
        lm = exact(lam.double().unsqueeze(1))
        oml = exact(1.0, like=Y).add(lm, 1, -1.0)
        b = oml.mul(exact(Y.double().index_select(0, partner)), 1)
        b = Interval(b.lo - TINY32, b.hi + TINY32)
        y = lm.fma(y, b)
    if smoothing != 0.0:
        eps = f32(smoothing)
        om = round32(torch.tensor(1.0 - eps, dtype=torch.float64, device=Y.device))
        y = exact(om).fma(y, exact(0.5 * eps, like=Y))
    return y


def batch_interval(rows_dev, den):
    """k_mlabel_batch's loss from the loss_rows the device stored (exact data): the double sum in a fixed order (relative D64 of
    sum|rows|; the centre is math.fsum's correctly rounded sum), one double division by den, ONE rounding to fp32"""
    r = rows_dev.detach().cpu().double().reshape(-1)
    S = torch.tensor(math.fsum(r.tolist()), dtype=torch.float64)
    Sa = torch.tensor(math.fsum(r.abs().tolist()), dtype=torch.float64)
    lo, hi = widen64((S - D64 * Sa) / den, (S + D64 * Sa) / den, 1)
    return Interval(round32(lo), round32(hi))


def mlabel_ex_intervals(z, Y, w, pw, N, C_, cfg, vec, partner=None, lam=None, reduction="mean", rows_dev=None):
    """Brackets of every output of mnas_mlabel_loss.  z, Y, w (None: no weights) fp32 [N][C], pw (None: no pos_weight) fp32 [C],
    partner int64 [N] / lam fp32 [N] (None: no mixing), as the device reads them; cfg = (gamma_pos, gamma_neg, margin, smoothing).
    The element is the general one iff a gamma, the margin or pos_weight is set, as the host decides it.
    -> dict(dl, ew, rows, row_half, t, [loss])."""
    gp, gn, m, eps = (f32(v) for v in cfg)
    z = z.double()
    t = label_intervals(Y, partner, lam, eps)
    one = exact(1.0, like=z)
    den = float(N) * float(C_) if reduction == "mean" else float(N)
    inv = exact(float(torch.tensor(1.0 / den, dtype=torch.float64).float()), like=z)
    ea = _f1(lambda x: torch.exp(x), exact(-z.abs()), clamp0=True)
    l1 = _f1(torch.log1p, ea, clamp0=True)
    d = one.add(ea, 1)
    q1, qe = one.div(d, 1, 2), ea.div(d, 1, 2)
    pos = z >= 0
    sg = _where(pos, q1, qe)
    wv = None if w is None else exact(w.double())
    if gp == 0.0 and gn == 0.0 and m == 0.0 and pw is None:
        # ml_bce on the interval t: A = max(z,0) - z*t fused (one rounding of the exact expression) or unfused (the product rounded
        # first), the hull; e = fl(A + l1); the row's term e*w exact inside a fused add or rounded, the hull
        mz, zt = exact(z.clamp_min(0.0)), exact(z).mul(t, 0)
        fused = mz.add(zt, 1, -1.0)
        zr = exact(z).mul(t, 1)
        unfused = mz.add(Interval(zr.lo - TINY32, zr.hi + TINY32), 1, -1.0)
        e = _hull(fused, unfused).add(l1, 1)
        if wv is None:
            ew = e
        else:
            ex, un = e.mul(wv, 0), e.mul(wv, 1)
            ew = Interval(torch.minimum(ex.lo, un.lo - TINY32), torch.maximum(ex.hi, un.hi + TINY32))
        g = sg.add(t, 1, -1.0)
        if wv is not None:
            g = _tiny(wv.mul(g, 1))
        dl = g.mul(inv, 1)
    else:
        oms = _where(pos, qe, q1)
        spp = exact(z.clamp_min(0.0)).add(l1, 1)
        spn = exact((-z).clamp_min(0.0)).add(l1, 1)
        # positive branch
        if gp != 0.0:
            G = exact(gp, like=z)
            ap = G.mul(spp, 1)
            Fp = _f1(torch.exp, _neg(ap), clamp0=True)
            ip = G.mul(sg, 1).fma(spn, oms)
            dpos = _neg(_tiny(Fp.mul(ip, 1)))
        else:
            Fp, dpos = one, _neg(oms)
        # negative branch
        if m == 0.0:
            Ln = spp
            if gn != 0.0:
                G = exact(gn, like=z)
                Fn = _f1(torch.exp, _neg(G.mul(spn, 1)), clamp0=True)
                inn = _tiny(G.mul(oms, 1)).fma(spp, sg)
                dneg = _tiny(Fn.mul(inn, 1))
            else:
                Fn, dneg = one, sg
        else:
            sm = sg.add(exact(m, like=z), 1, -1.0)
            live, dead = sm.hi > 0, sm.lo <= 0              # may, may not take the live side
            sl = Interval(sm.lo.clamp_min(TINY32), sm.hi.clamp_min(TINY32))
            om = one.add(sl, 1, -1.0)
            Lnl = _neg(_f1(torch.log1p, _neg(sl)))
            Lnl = Interval(Lnl.lo.clamp_min(0.0), Lnl.hi)
            if gn != 0.0:
                G = exact(gn, like=z)
                lsm = _f1(torch.log, sl)
                Fnl = _f1(torch.exp, _tiny(G.mul(lsm, 1)), clamp0=True)
                e1 = _f1(torch.exp, _tiny(exact(gn - 1.0, like=z).mul(lsm, 1)), clamp0=True)
                P1 = _tiny(G.mul(e1, 1))
                Fnd = 0.0
            else:
                Fnl, P1, Fnd = one, exact(0.0, like=z), 1.0
            qn = Fnl.div(om, 1, 2)
            inn = P1.fma(Lnl, qn)
            dnl = _tiny(_tiny(sg.mul(oms, 1)).mul(inn, 1))
            zero = _full(0.0, z)
            Fn = _pick(live, dead, Fnl, _full(Fnd, z))
            Ln = _pick(live, dead, Lnl, zero)
            dneg = _pick(live, dead, dnl, zero)
        p = one if pw is None else exact(pw.double().unsqueeze(0).expand_as(z))
        pt = t if pw is None else _tiny(p.mul(t, 1))
        omt = one.add(t, 1, -1.0)
        ep = _tiny(pt.mul(_tiny(Fp.mul(spn, 1)), 1))
        fn = _tiny(Fn.mul(Ln, 1))
        e = omt.fma(fn, ep)
        ew = e if wv is None else e.mul(wv, 0)              # fmaf(e, w, ls): the product is exact inside the add
        g = omt.fma(dneg, _tiny(pt.mul(dpos, 1)))
        if wv is not None:
            g = _tiny(wv.mul(g, 1))
        dl = g.mul(inv, 1)
    dl = _tiny(dl)
    T = mlabel_trips(C_, vec)
    row_half = (T + 9) * 2.0 ** -23 * ew.amax.sum(1) + ew.half.sum(1)
    rows = Interval(ew.mid.sum(1) - row_half, ew.mid.sum(1) + row_half)
    out = dict(dl=dl, ew=ew, rows=rows, row_half=row_half, t=t)
    if rows_dev is not None:
        out["loss"] = batch_interval(rows_dev, den)
    return out


def _tiny(iv):
    """the absolute floor of a rounding whose result may be subnormal (Interval.mul does not add it)"""
    return Interval(iv.lo - TINY32, iv.hi + TINY32)


def _pick(live, dead, a, b):
    """a where only the live side can be taken, b where only the dead one, the hull where both"""
    both = _hull(a, b)
    return _where(live & dead, both, _where(live, a, b))


def check_rows(rows_dev, iv, what):
    """the device's loss_rows inside the rows bracket (check_sum_bound's form) -> worst error / bound"""
    r = rows_dev.double()
    mid, half = iv["rows"].mid.to(r.device), iv["row_half"].to(r.device) + TINY32
    err = (r - mid).abs()
    assert bool((err <= half).all()), "%s: a row sum outside its bound (worst x%.2f)" % (what, float((err / half).max()))
    return float((err / half).max())
