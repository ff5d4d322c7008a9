"""Per-element bounds for the distillation cross-entropy kernels (csrc/mnas_head.hip: k_head_ce_kd, k_head_loss_mean_kd).
Conventions of intervals.py; the propagation follows the operation order written above k_head_ce_kd, in its uncontracted form, and
rests on the one assumption bounds_tail.ce_intervals rests on: OCML expf / logf and the divisions at one ULP."""
import torch

from gpu_util import L
from intervals import D64, TINY32, U32, Interval, check_interval, widen

exact = Interval.exact
F32 = lambda v: torch.tensor(v, dtype=torch.float32)


def _col(iv):
    return Interval(iv.lo[:, None], iv.hi[:, None])


def _rounded(lo, hi, n=1):
    return Interval(*widen(lo, hi, n, floor=True))


def _exp(d):
    """expf of a finite argument in [d.lo, d.hi]: one ulp, and an exponential below 2^-126 may come out as zero"""
    lo = (torch.exp(d.lo) * (1 - 2 * U32 - D64) - 2.0 ** -126).clamp_min(0.0)
    return Interval(lo, torch.exp(d.hi) * (1 + 2 * U32 + D64) + 2.0 ** -126)


def _log(s):
    """logf of a positive argument in [s.lo, s.hi]: one ulp"""
    lo, hi = widen(torch.log(s.lo), torch.log(s.hi), 1, 2, host=D64)
    return Interval(lo - D64, hi + D64)


def _sum_pos(t, n, dim):
    """the fp32 sum of non-negative terms in n adds: relative (1 + u)^n"""
    return Interval(*widen(t.lo.sum(dim), t.hi.sum(dim), n))


def _sum_signed(t, n, dim):
    """the fp32 sum of signed terms in n adds: within ((1 + u)^n - 1) sum |term| of the exact sum"""
    f = (1 + U32) ** n - 1
    sa = t.amax.sum(dim)
    return Interval(t.lo.sum(dim) - f * sa - n * TINY32, t.hi.sum(dim) + f * sa + n * TINY32)


def kd_settings(eps, T, alpha):
    """the fp32 scalars of a call, as the C ABI passes them and as the kernels form them (each one deterministic fp32 operation of
    exact data, reproduced bit for bit): eps, 1 - eps, alpha, 1 - alpha, T, alpha T, T T"""
    e, t, a = F32(eps), F32(T), F32(alpha)
    one = F32(1.0)
    return dict(eps=float(e), ome=float(one - e), alpha=float(a), oma=float(one - a), T=float(t), aT=float(a * t), T2=float(t * t))


def kd_intervals(z, ta, tb=None, lam=None, eps=0.0, w=None, t=None, T=1.0, alpha=0.5, ignore_index=-100):
    """Brackets of dlogits (N, C), of the hard and distillation loss rows (N,) each and of D, for FINITE logits z, t (the edge rules
    with infinities are asserted one by one in the tests).  Every operation of the kernel's documented order is one rounding (u),
    expf / logf / divisions two; a sum is widened by its ceil(n / 256) + 9 adds.  Scalars that are one fp32 operation of exact
    data (1 - eps, 1 - alpha, alpha T) enter bit for bit (kd_settings).  Ignored rows: hard row and hard gradient exactly 0;
    refused rows: dlogits exactly 0, both rows NaN (`nan_rows`).  D == 0 (every row ignored, or only zero weights counted): hard
    gradient exactly 0, hard mean NaN.  -> dict(dl, hard_rows, kd_rows, D (Interval or None), valid, nan_rows, kd (bool))."""
    x = z.double()
    N, Cn = x.shape
    assert bool(torch.isfinite(x).all()) and (t is None or bool(torch.isfinite(t).all()))
    st = kd_settings(eps, T, alpha)
    kd = t is not None and st["alpha"] != 0.0
    hard_on = not (kd and st["alpha"] == 1.0)
    b = ta if tb is None else tb
    l32 = torch.ones(N, dtype=torch.float32) if (tb is None or lam is None) else lam.float()
    ignored = (ta == ignore_index) | (b == ignore_index)
    inrange = (ta >= 0) & (ta < Cn) & (b >= 0) & (b < Cn) & (l32 >= 0) & (l32 <= 1)
    valid, refused = ~ignored & inrange, ~ignored & ~inrange
    a0, b0 = torch.where(valid, ta, torch.zeros_like(ta)), torch.where(valid, b, torch.zeros_like(b))
    rowi = torch.arange(N)
    same = ta == b
    l = exact(torch.where(valid, l32, torch.ones_like(l32)).double())
    zero_n, one_n = torch.zeros(N, dtype=torch.float64), torch.ones(N, dtype=torch.float64)
    nC, nN = -(-Cn // 256) + 9, -(-N // 256) + 9
    one = exact(1.0)
    cdiv = lambda iv: iv.div(exact(float(Cn)), 1, 2)

    # ---- row weights s_i and the divisor D
    if w is None:
        wA = wB = exact(one_n)
        sn = exact(one_n)
        s_all = exact((~ignored).double())                    # (a refused row counts, as in k_head_ce_soft; its NaN row poisons the mean)
        D = exact(s_all.lo.sum())                             # an integer < 2^24: exact in any order
        Wm = one
    else:
        wd = w.double()
        wA, wB = exact(wd[a0]), exact(wd[b0])
        mixed = l.fma(wA.add(wB, 1, -1.0), wB)
        sn = Interval(torch.where(same, wA.lo, mixed.lo), torch.where(same, wA.hi, mixed.hi))
        vm = valid.double()
        s_all = Interval(sn.lo * vm, sn.hi * vm)
        D = _sum_pos(Interval(s_all.lo.clamp_min(0.0), s_all.hi.clamp_min(0.0)), nN, 0)
        Wm = cdiv(_sum_pos(exact(wd), nC, 0))
    d_pos = bool(D.lo > 0)
    assert d_pos or bool(D.hi <= 0), "D straddles 0: not a case for the bracket"
    invD = one.div(D, 1, 2) if d_pos else exact(0.0)

    # ---- the softmax of the hard term
    mx = x.max(1, keepdim=True).values
    d = _rounded(x - mx, x - mx)
    e = _exp(d)
    se = _sum_pos(e, nC, 1)
    p = e.mul(_col(one.div(se, 1, 2)), 1)

    # ---- the target row q and its weighted form
    ome = exact(st["ome"])
    wa_m = ome.mul(l, 1)
    wb_m = ome.add(wa_m, 1, -1.0)
    full = torch.full((N,), st["ome"], dtype=torch.float64)
    wa = Interval(torch.where(same, full, wa_m.lo), torch.where(same, full, wa_m.hi))
    wb = Interval(torch.where(same, zero_n, wb_m.lo), torch.where(same, zero_n, wb_m.hi))
    qlo, qhi = torch.zeros_like(x), torch.zeros_like(x)
    qlo[rowi, a0], qhi[rowi, a0] = wa.lo, wa.hi
    ns = ~same
    qlo[rowi[ns], b0[ns]], qhi[rowi[ns], b0[ns]] = wb.lo[ns], wb.hi[ns]
    q = Interval(qlo, qhi)
    if st["eps"] != 0.0:
        q = q.add(cdiv(exact(st["eps"])), 1)
    if w is None:
        wq, S = q, exact(one_n)
    else:
        wq = exact(wd[None, :]).mul(q, 1)
        S = exact(st["eps"]).fma(Wm.add(sn, 1, -1.0), sn)
    ch = exact(st["oma"]).mul(invD, 1) if kd else invD
    g = p.mul(_col(S), 1).add(wq, 1, -1.0).mul(ch, 1)
    gm = (valid[:, None] if (hard_on and d_pos) else torch.zeros((N, 1), dtype=torch.bool)).double()
    g = Interval(g.lo * gm, g.hi * gm)

    # ---- the loss row of the hard term
    lse = _log(se).add(exact(mx[:, 0]), 1)
    za, zb = exact(x[rowi, a0]), exact(x[rowi, b0])
    waA, wbB = (wa, wb) if w is None else (wa.mul(wA, 1), wb.mul(wB, 1))
    hard = waA.mul(lse.add(za, 1, -1.0), 1).add(wbB.mul(lse.add(zb, 1, -1.0), 1), 1)
    if st["eps"] != 0.0:
        terms = exact(x) if w is None else exact(wd[None, :] * x)            # (the product is inside the fma: exact)
        swz = _sum_signed(terms, nC, 1)
        sm = (lse if w is None else Wm.mul(lse, 1)).add(cdiv(swz), 1, -1.0)
        hard = hard.add(exact(st["eps"]).mul(sm, 1), 1)
    hard = Interval(torch.where(valid, hard.lo, zero_n), torch.where(valid, hard.hi, zero_n))

    # ---- the distillation term
    kd_rows = exact(zero_n)
    if kd:
        tt = t.double()
        invT = one.div(exact(st["T"]), 1, 2)
        mt = tt.max(1, keepdim=True).values
        dt = _rounded(tt - mt, tt - mt)
        eS, eT = _exp(d.mul(invT, 1)), _exp(dt.mul(invT, 1))
        seS, seT = _sum_pos(eS, nC, 1), _sum_pos(eT, nC, 1)
        rseT = one.div(seT, 1, 2)
        pS, pT = eS.mul(_col(one.div(seS, 1, 2)), 1), eT.mul(_col(rseT), 1)
        ck = exact(st["aT"]).div(exact(float(N)), 1, 2)
        g = g.add(ck.mul(pS.add(pT, 1, -1.0), 1), 1)
        sA = _sum_signed(eT.mul(dt.add(d, 1, -1.0), 1), nC, 1)
        kd_rows = sA.mul(rseT, 1).mul(invT, 1).add(_log(seS).add(_log(seT), 1, -1.0), 1)
    rm = (~refused)[:, None].double()
    dl = Interval(g.lo * rm, g.hi * rm)
    return dict(dl=dl, hard_rows=hard, kd_rows=kd_rows, D=D if d_pos else None, valid=valid, nan_rows=refused, kd=kd, settings=st)


def kd_mean_intervals(rows_dev, parts_dev, iv, N):
    """k_head_loss_mean_kd from what the device stored (exact data): hard = sum(hard rows) / D with D's own bracket, kd = fl(T T)
    fl(sum(kd rows) / N), each sum in ceil(N / 256) + 9 adds; the total from the two stored parts: fl(fl((1 - alpha) hard) +
    fl(alpha kd)), hard alone without the distillation term, kd alone at alpha == 1.  -> (hard, kd, total) Intervals, None where
    the value is NaN by rule (D == 0; a NaN part)."""
    st = iv["settings"]
    r = rows_dev.double()
    nN = -(-N // 256) + 9
    hard = kdv = None
    if iv["D"] is not None:
        hard = _sum_signed(exact(r[:N]), nN, 0).div(iv["D"], 1, 2)
    if iv["kd"]:
        kdv = exact(st["T2"]).mul(_sum_signed(exact(r[N:]), nN, 0).div(exact(float(N)), 1, 2), 1)
    else:
        kdv = exact(0.0)
    ph, pk = parts_dev.double()
    if not iv["kd"]:
        total = None if bool(torch.isnan(ph)) else exact(ph)
    elif st["alpha"] == 1.0:
        total = None if bool(torch.isnan(pk)) else exact(pk)
    elif bool(torch.isnan(ph) | torch.isnan(pk)):
        total = None
    else:
        total = exact(st["oma"]).mul(exact(ph), 1).add(exact(st["alpha"]).mul(exact(pk), 1), 1)
    return hard, kdv, total


def check_kd(dl, rows, parts, loss, iv, what, family="distillation cross-entropy"):
    """EVERY dlogits element, both halves of loss_rows and the three means inside their brackets (host tensors of one call).
    -> worst error / bracket.  Raises AssertionError on the first output outside."""
    N = iv["valid"].numel()
    rows, parts, loss = rows.double(), parts.double(), loss.double().reshape(())
    nan = iv["nan_rows"]
    assert bool(torch.isnan(rows[:N][nan]).all()), what + ": a refused row's hard loss must be NaN"
    if iv["kd"]:
        assert bool(torch.isnan(rows[N:][nan]).all()), what + ": a refused row's distillation loss must be NaN"
    ok = ~nan
    sub = lambda v, m: Interval(v.lo[m], v.hi[m])
    worst = [check_interval(dl, iv["dl"], what + " dlogits", family),
             check_interval(rows[:N][ok], sub(iv["hard_rows"], ok), what + " hard rows", family),
             check_interval(rows[N:][ok], sub(iv["kd_rows"], ok), what + " kd rows", family)]
    hard, kdv, total = kd_mean_intervals(rows, parts, iv, N)
    poisoned = bool(nan.any())
    for name, got, want, isnan in (("hard", parts[0], hard, poisoned or hard is None),
                                   ("kd", parts[1], kdv, poisoned and iv["kd"]),
                                   ("loss", loss, total, total is None)):
        if isnan:
            assert bool(torch.isnan(got)), "%s %s: outside the per-element bound (NaN expected, got %r)" % (what, name, float(got))
        else:
            worst.append(check_interval(got, want, "%s %s mean" % (what, name), family + " mean" if family else None))
    return max(worst)


class KD:
    """the raw mnas_head_cross_entropy_kd call with its own scratch; every output in a guarded buffer (gpu_util.guarded)"""

    def __init__(self, N, Cn):
        from gpu_util import guarded
        self.N, self.Cn = N, Cn
        self.dl, self._dl = guarded((N, Cn), torch.float32)
        self.rows, self._rows = guarded((2 * N,), torch.float32)
        self.parts, self._parts = guarded((2,), torch.float32)
        self.loss, self._loss = guarded((1,), torch.float32)
        self.bad, self._bad = guarded((1,), torch.int32)
        self.ranks, self._ranks = guarded((N,), torch.int32)
        self.fill()

    def fill(self):
        for t in (self.dl, self.rows, self.parts, self.loss):
            t.fill_(float("nan"))
        self.bad.zero_()

    def args(self, z, a, b, lam, eps, w, t, T, alpha, meters=None, grad=True, ignore=-100, parts=True):
        ks, nk, ranks, blk = (None, 0, 0, 0) if meters is None else meters.kernel_args(self.N, z.device)
        if meters is not None:
            ranks = self.ranks.data_ptr()
        return (z.data_ptr(), L.ptr(a), L.ptr(b), L.ptr(lam), eps, L.ptr(w), L.ptr(t), T, alpha, self.N, self.Cn, ignore,
                self.rows.data_ptr(), self.loss.data_ptr(), self.parts.data_ptr() if parts else 0, self.dl.data_ptr() if grad else 0,
                self.bad.data_ptr(), ks, nk, ranks, blk, L.cur_stream())

    def run(self, z, a, b=None, lam=None, eps=0.0, w=None, t=None, T=1.0, alpha=0.5, what="kd", **kw):
        """-> dict of host tensors dl, rows, parts, loss and the flag; the canaries around every output checked"""
        self.fill()
        L.check(L.load().mnas_head_cross_entropy_kd(*self.args(z, a, b, lam, eps, w, t, T, alpha, **kw)), what)
        self._dl(what + " dlogits", written=False)
        self._rows(what + " loss_rows", written=False)
        self._parts(what + " loss_parts", written=False)
        self._loss(what + " loss", written=False)
        self._bad(what + " bad_flag", written=False)
        self._ranks(what + " rank_rows", written=False)
        return dict(dl=self.dl.cpu(), rows=self.rows.cpu(), parts=self.parts.cpu(), loss=self.loss.cpu()[0], bad=int(self.bad))
