"""Per-element bounds for the fp32 tail of the step: classifier-head GEMMs, cross-entropy, flat-buffer optimizers.
Conventions of intervals.py.  The references are fp64 arithmetic on the fp32 values the device reads; host-side scalars
(drop_scale, Adam's bias corrections, lr / bc1) are reproduced bit for bit in float32 and enter as exact data."""
import ctypes as C

import torch

from gpu_util import L, bits_equal, guarded
from intervals import D64, TINY32, U32, Interval, _assert_bound, check_interval, f32, widen

exact = Interval.exact


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _pow2(n, seed, lo, hi):
    """n exact powers of two 2^k, k uniform in [lo, hi]"""
    k = torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed))
    return torch.pow(torch.tensor(2.0), k.float())


# ---- classifier-head GEMMs (csrc/mnas_head.hip: k_head_gemm) -------------------------------------------------------------------------
HEAD_SIZES = [(256, 320, 512), (37, 320, 1000), (5, 512, 10), (64, 256, 1000), (130, 70, 65),
              (1, 1, 1), (1, 129, 1), (33, 128, 33), (32, 127, 32)]
HEAD_PS = [0.0, 0.5, 0.2, 0.999]


def head_chain(K):
    """fmaf per output and wave: every K step of 128 gives each of the 8 waves 16 k, zero-padded steps included"""
    return 16 * -(-K // 128)


def head_drop_scale(p):
    """head_drop: (float)(1.0 / (1.0 - (double)p)) of the fp32 p the ABI passes"""
    return float(torch.tensor(1.0 / (1.0 - f32(p)), dtype=torch.float64).float())


def head_dropped(x, keep, p):
    """the operand under dropout as k_head_gemm stages it: the single fp32 product x * drop_scale (stored to LDS before any
    FMA, so nothing contracts into it) where kept, 0 elsewhere -- reproduced bit for bit by a float32 multiply"""
    if p == 0:
        return x.clone()
    sc = torch.tensor(head_drop_scale(p), dtype=torch.float32)
    return torch.where(keep, x * sc, torch.zeros_like(x))


def head_gemm_interval(A, B, bias=None, C0=None, relu=False, post=None, mask=None):
    """Bracket of one k_head_gemm output tile set: A (M, K), B (K, N) the fp32 operands AS STAGED (head_dropped applied), bias [N],
    C0 the accumulate target, post (M, N) the exact epilogue factor keep * drop_scale of drop_where == 3, mask the exact 0/1
    ReLU mask of bwd_x.  Roundings on the way of any term to the stored value, each at most u of a running magnitude <= S:
      L = 16 * ceil(K / 128) fmaf of the wave's chain (head_chain), 7 adds of the eight partial tiles in wave order (the first, to
      0.f, is exact), the bias add, the drop_where == 3 multiply, the accumulate add: L + 10 counting the exact first add;
      ReLU and mask are exact.  ref = A B + bias (times post) + C0 in fp64, S the same over absolute values; doubled as in
      check_gemm_bound (it absorbs every second-order term):   |hip - ref| <= (L + 10) * 2^-23 * S   for EVERY element.
    The ReLU is monotone: it is applied to the bracket's two ends, no element is excluded; a masked element is exactly 0."""
    A, B = A.double(), B.double()
    K = A.shape[1]
    ref, S = A @ B, A.abs() @ B.abs()
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if post is not None:
        ref, S = ref * post.double(), S * post.double().abs()
    if C0 is not None:
        ref, S = ref + C0.double(), S + C0.double().abs()
    b = (head_chain(K) + 10) * 2.0 ** -23 * S
    lo, hi = ref - b, ref + b
    if relu:
        lo, hi = torch.relu(lo), torch.relu(hi)
    if mask is not None:
        lo, hi = lo * mask.double(), hi * mask.double()
    return Interval(lo, hi)


def head_rowsum_interval(A, r0=None):
    """Bracket of rowsum[m] (+)= sum_k A(m, k) (db of bwd_w): per wave and K step `asum += (a0 + a1) + (a2 + a3)` for each of its
    four groups of four k -- a term passes 2 roundings inside its group and at most 4 * ceil(K / 128) adds of the running sum --,
    then 7 adds of the eight waves' sums (first exact) and the accumulate add: (4 * ceil(K / 128) + 10) roundings, doubled:
        |hip - ref| <= (4 * ceil(K / 128) + 10) * 2^-23 * S,   S = sum_k |A(m, k)| + |r0|."""
    A = A.double()
    ref, S = A.sum(1), A.abs().sum(1)
    if r0 is not None:
        ref, S = ref + r0.double(), S + r0.double().abs()
    b = (4 * -(-A.shape[1] // 128) + 10) * 2.0 ** -23 * S
    return Interval(ref - b, ref + b)


def head_inputs(N, I, O_, scaled, seed=0):
    """(x, w, b, dz, u_prev, c0w, c0b) of the head GEMM bound tests (also read by tests/test_bounds_cpu.py).  scaled: rows and
    columns of every operand times exact powers of two 2^-12 .. 2^12 (a scale per batch row, per input and per output feature;
    w carries out / in, so that no product of the reduction cancels a scale), most outputs then lie far below the tensor's maximum;
    u_prev (the ReLU mask source) holds exact +0.0, -0.0 and the smallest positive subnormal."""
    x, w, b = _rand((N, I), seed + 1), _rand((O_, I), seed + 2) * 0.1, _rand((O_,), seed + 3)
    dz, u_prev = _rand((N, O_), seed + 4), _rand((N, I), seed + 5)
    c0w, c0b = _rand((O_, I), seed + 6) * 0.25, _rand((O_,), seed + 7) * 0.5
    if scaled:
        rn, ri, ro = _pow2(N, seed + 8, -12, 12), _pow2(I, seed + 9, -12, 12), _pow2(O_, seed + 10, -12, 12)
        x, w, b, dz = x * rn[:, None] * ri, w * ro[:, None] / ri, b * ro, dz * rn[:, None] * ro
        c0w, c0b = c0w * ro[:, None] * ri, c0b * ro
    flat = u_prev.view(-1)
    flat[0::7] = 0.0
    flat[1::7] = -0.0
    flat[2::7] = 2.0 ** -149
    return x, w, b, dz, u_prev, c0w, c0b


HEAD_LIVE_K = lambda K: sorted({k for k in (0, 15, 16, 127, 128, K - 1) if 0 <= k < K})
HEAD_PROBE_RC = lambda M: sorted({r for r in (0, 31, 32, M - 1) if 0 <= r < M})


def head_sparse(t, dim, K):
    """t with everything zero along `dim` except the live k"""
    out = torch.zeros_like(t)
    idx = torch.tensor(HEAD_LIVE_K(K))
    out.index_copy_(dim, idx, t.index_select(dim, idx))
    return out


def head_probe_visible(A, B, iv, what):
    """each live term's contribution |A(m,k) B(k,n)| exceeds twice the bound at some probed (row, column)"""
    A, B = A.double(), B.double()
    rows, cols = torch.tensor(HEAD_PROBE_RC(A.shape[0])), torch.tensor(HEAD_PROBE_RC(B.shape[1]))
    half = iv.half.cpu()[rows][:, cols]
    for k in HEAD_LIVE_K(A.shape[1]):
        term = (A[rows, k].abs()[:, None] * B[k, cols].abs()[None, :])
        assert bool((term > 2 * half).any()), "%s: live k = %d would not be seen" % (what, k)


# ---- cross-entropy, plain and soft (k_head_ce, k_head_ce_soft, the mean stages) -------------------------------------------------------
CE_SIZES = [(1, 1), (33, 1), (1, 1000), (7, 255), (7, 256), (7, 513), (257, 10), (600, 257)]
CE_ROWS = ["uniform4", "uniform40", "peak_on", "peak_off", "equal", "plus1000", "minus1000", "neg_inf"]
CE_IGNORE = ["none", "third", "all_but_one", "all"]


def ce_targets(N, Cn):
    i = torch.arange(N)
    return (i * 7 + 3) % Cn, (i * 5 + 1) % Cn


def ce_logits(kind, N, Cn, seed=11):
    """the logit rows of the cross-entropy bound tests; labels are ce_targets' (neg_inf spares both)"""
    u = _rand((N, Cn), seed)
    a, b = ce_targets(N, Cn)
    if kind == "uniform4":
        return u * 4
    if kind == "uniform40":
        return u * 40
    if kind in ("peak_on", "peak_off"):
        z = u.clone()
        at = a if kind == "peak_on" else (a + 1) % Cn
        z[torch.arange(N), at] += 30.0
        return z
    if kind == "equal":
        return torch.full((N, Cn), 0.75)
    if kind == "plus1000":
        return u * 4 + 1000.0
    if kind == "minus1000":
        return u * 4 - 1000.0
    assert kind == "neg_inf"
    z = u * 4
    m = (torch.arange(Cn)[None, :] + torch.arange(N)[:, None]) % 3 == 0
    m[torch.arange(N), a] = False
    m[torch.arange(N), b] = False
    z[m] = float("-inf")
    return z


def ce_ignore(t, how, ignore_index=-100):
    t = t.clone()
    if how == "third":
        t[::3] = ignore_index
    elif how == "all_but_one":
        kept = int(t[t.numel() // 2])
        t[:] = ignore_index
        t[t.numel() // 2] = kept
    elif how == "all":
        t[:] = ignore_index
    return t


def ce_intervals(x, ta, tb=None, lam=None, eps=None, ignore_index=-100):
    """Brackets of dlogits (N, C) and loss_rows (N,) of k_head_ce (eps None) / k_head_ce_soft, by interval propagation through
    the kernel's operations in their UNCONTRACTED form.  csrc/mnas_head.hip is built with -ffp-contract=fast and without any
    fast-math flag: a contracted form (p - q as one fma of e and rse, the loss row's products folded into its sums) rounds less
    often and lies inside the bracket of the uncontracted one.  x fp32 as the device reads it; every operation one rounding (u):
      mx = max_c x (exact); d = fl(x - mx); e = expf(d); se = sum_c e in ceil(C/256) + 9 adds of non-negative terms (the lane's
      strided sum, six butterfly levels, three adds of the four waves): relative (1 + u)^n; rse = 1/se; p = fl(e rse);
      plain: q = [c == t]; soft: wa = fl(1-eps) or fl(fl(1-eps) lam), wb = 0 or fl(fl(1-eps) - wa) (bracketed, so that the fma
      a compiler may form of it is inside), uq = eps/C, q = fl((qa + qb) + uq) -- the first add always has a zero operand --;
      dlogits = fl(fl(p - q) inv), inv = 1/count, count (rows not ignored) exact.
      loss row, plain: fl(fl(logf(se) + mx) - x[t]); soft: lse = fl(logf(se) + mx), fl(fl(fl(wa fl(lse - x[a])) + fl(wb fl(lse -
      x[b]))) + fl(eps fl(lse - fl(sz/C)))) with sz = sum_c x in the same ceil(C/256) + 9 adds (signed terms: absolute
      ((1 + u)^n - 1) sum|x|); with eps == 0 the smoothing term is left out (the kernel multiplies 0 by 0).
    expf, logf and the three divisions are taken at ONE ULP (2u relative): HIP's documented accuracy of these OCML functions,
    the one assumption here that IEEE 754 does not give; an exponential below 2^-126 may come out as zero (+-2^-126).  The tests
    print the measured error / bracket ratio, which is the check of that assumption.  A -inf logit has e = 0 exactly; with
    eps > 0 it makes the row's loss +inf (the smoothing term reads every class).  Ignored and refused rows: dlogits exactly 0;
    loss row 0 resp. NaN (`nan_rows`).  -> dict(dl=Interval, rows=Interval over all rows (0 at invalid ones), valid, nan_rows,
    count)."""
    x = x.double()
    N, Cn = x.shape
    dev = x.device
    ta = ta.to(dev)
    b = ta if tb is None else tb.to(dev)
    l32 = torch.ones(N, dtype=torch.float32, device=dev) if (tb is None or lam is None) else lam.to(dev).float()
    ignored = (ta == ignore_index) | (b == ignore_index)
    inrange = (ta >= 0) & (ta < Cn) & (b >= 0) & (b < Cn) & (l32 >= 0) & (l32 <= 1)
    valid = ~ignored & inrange
    count = int((~ignored).sum())
    a0, b0 = torch.where(valid, ta, torch.zeros_like(ta)), torch.where(valid, b, torch.zeros_like(b))
    rowi = torch.arange(N, device=dev)
    neg = torch.isinf(x) & (x < 0)
    mx = x.max(1, keepdim=True).values
    dlo, dhi = widen(torch.where(neg, mx, x) - mx, torch.where(neg, mx, x) - mx, 1, floor=True)
    elo = (torch.exp(dlo) * (1 - 2 * U32 - D64) - 2.0 ** -126).clamp_min(0.0)
    ehi = torch.exp(dhi) * (1 + 2 * U32 + D64) + 2.0 ** -126
    elo, ehi = torch.where(neg, torch.zeros_like(elo), elo), torch.where(neg, torch.zeros_like(ehi), ehi)
    nadd = -(-Cn // 256) + 9
    se = Interval(*widen(elo.sum(1, keepdim=True), ehi.sum(1, keepdim=True), nadd))
    one = exact(1.0, like=x)
    rse = one.div(se, 1, 2)
    p = Interval(elo, ehi).mul(rse, 1)
    inv = one.div(exact(float(max(count, 1)), like=x), 1, 2)
    # the target row q
    if eps is None:
        e32, ome = 0.0, 1.0
        wa = exact(torch.ones(N, dtype=torch.float64, device=dev))
        wb = exact(torch.zeros(N, dtype=torch.float64, device=dev))
        same = torch.ones(N, dtype=torch.bool, device=dev)
    else:
        e32 = f32(eps)
        ome = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(e32, dtype=torch.float32))
        same = ta == b
        wa_m = exact(ome, like=x).mul(exact(l32.double()), 1)
        wb_m = exact(ome, like=x).add(wa_m, 1, -1.0)
        full, zero = torch.full((N,), ome, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
        wa = Interval(torch.where(same, full, wa_m.lo), torch.where(same, full, wa_m.hi))
        wb = Interval(torch.where(same, zero, wb_m.lo), torch.where(same, zero, wb_m.hi))
    qlo, qhi = torch.zeros_like(x), torch.zeros_like(x)
    qlo[rowi, a0], qhi[rowi, a0] = wa.lo, wa.hi
    ns = ~same
    qlo[rowi[ns], b0[ns]], qhi[rowi[ns], b0[ns]] = wb.lo[ns], wb.hi[ns]
    q = Interval(qlo, qhi)
    if e32 != 0.0:
        q = q.add(exact(e32, like=x).div(exact(float(Cn), like=x), 1, 2), 1)
    dl = p.add(q, 1, -1.0).mul(inv, 1)
    vm = valid[:, None].double() if count > 0 else torch.zeros((N, 1), dtype=torch.float64, device=dev)
    dl = Interval(dl.lo * vm, dl.hi * vm)
    # the loss row
    lg_lo, lg_hi = widen(torch.log(se.lo), torch.log(se.hi), 1, 2, host=D64)
    lse = Interval(lg_lo - D64, lg_hi + D64).add(exact(mx), 1)
    lse = Interval(lse.lo[:, 0], lse.hi[:, 0])
    zero_n = torch.zeros(N, dtype=torch.float64, device=dev)
    za, zb = exact(torch.where(valid, x[rowi, a0], zero_n)), exact(torch.where(valid, x[rowi, b0], zero_n))
    if eps is None:
        rows = lse.add(za, 1, -1.0)
    else:
        m1 = wa.mul(lse.add(za, 1, -1.0), 1)
        m2 = wb.mul(lse.add(zb, 1, -1.0), 1)
        rows = m1.add(m2, 1)
        if e32 != 0.0:
            xf = torch.where(neg, torch.zeros_like(x), x)
            s, sa = xf.sum(1), xf.abs().sum(1)
            fs = (1 + U32) ** nadd - 1
            szc = Interval(s - fs * sa, s + fs * sa).div(exact(float(Cn), like=x), 1, 2)
            rows = rows.add(exact(e32, like=x).mul(lse.add(szc, 1, -1.0), 1), 1)
            anyneg = neg.any(1)
            inf = torch.full((N,), float("inf"), dtype=torch.float64, device=dev)
            rows = Interval(torch.where(anyneg, inf, rows.lo), torch.where(anyneg, inf, rows.hi))
    z = torch.zeros(N, dtype=torch.float64, device=dev)
    rows = Interval(torch.where(valid, rows.lo, z), torch.where(valid, rows.hi, z))
    return dict(dl=dl, rows=rows, valid=valid, nan_rows=~ignored & ~inrange, count=count)


def ce_mean_interval(rows_dev, count):
    """k_head_loss_mean(_soft) from the loss_rows the device stored (exact data; ignored rows hold 0): the lane's strided sum,
    the butterfly and the four waves are ceil(N/256) + 9 adds -- within ((1 + u)^n - 1) sum|rows| of the exact sum --, then one
    division (one ulp) by the count, which is an exact integer in fp32.  count == 0: 0/0, NaN (returns None)."""
    if count == 0:
        return None
    r = rows_dev.double()
    n = -(-r.numel() // 256) + 9
    s, sa = r.sum(), r.abs().sum()
    f = (1 + U32) ** n - 1
    return Interval(s - f * sa, s + f * sa).div(exact(float(count), like=r), 1, 2)


def check_ce_mean(loss, rows_dev, count, what, family):
    """the mean against ce_mean_interval; no row counted: NaN; a +inf row (a -inf logit under smoothing): +inf; a NaN row (a
    refused label): NaN"""
    loss = loss.detach().double().cpu().reshape(())
    r = rows_dev.detach().double().cpu()
    if count == 0 or bool(torch.isnan(r).any()):
        assert bool(torch.isnan(loss)), "%s: outside the per-element bound (NaN expected, got %r)" % (what, float(loss))
        return 0.0
    if not bool(torch.isfinite(r).all()):
        assert float(loss) == float(r.sum()), "%s: outside the per-element bound (%r expected, got %r)" % (what, float(r.sum()), float(loss))
        return 0.0
    return check_interval(loss, ce_mean_interval(r, count), what, family)


# ---- flat-buffer optimizers (csrc/mnas_elementwise.hip: k_adam, k_rmsprop, k_sgd and the _ex variants) ---------------------------------
OPT_SIZES = [1, 255, 257, 10007, 2048 * 256 + 300]
OPT_GRID_CAP = 2048 * 256          # opt_blocks: at most 2048 workgroups of 256 lanes; beyond it a lane takes a second trip


def opt_data(n, seed=0):
    """(p, g, m, v, buf) fp32: p, g with per-element power-of-two scales 2^-20 .. 2^4, both signs and exact zeros; m, buf
    non-zero of either sign; v > 0 except: every 11th element has v = 0 AND g = 0 (denom = eps), every 13th a tiny v = 1e-30"""
    p = _rand((n,), seed + 1) * _pow2(n, seed + 2, -20, 4)
    g = _rand((n,), seed + 3) * _pow2(n, seed + 4, -20, 4)
    m = _rand((n,), seed + 5) * 0.1 + 0.01
    buf = _rand((n,), seed + 6) * 0.1 - 0.01
    v = _rand((n,), seed + 7).abs() * 1e-2 + 1e-6
    p[3::17] = 0.0
    g[5::19] = 0.0
    v[7::13] = 1e-30
    v[0::11] = 0.0
    g[0::11] = 0.0
    return p, g, m, v, buf


def adam_bias(b1, b2, step):
    """(bc1, sqrtf(bc2)) as mnas_adam_step forms them: 1.f - powf(beta, (float)step) with the C library's powf (numpy's float32
    power may take another route), a float32 square root"""
    import ctypes.util
    import numpy as np
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.powf.restype, libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    one = np.float32(1.0)
    bc1 = one - np.float32(libm.powf(C.c_float(b1), C.c_float(float(step))))
    bc2 = one - np.float32(libm.powf(C.c_float(b2), C.c_float(float(step))))
    return float(bc1), float(np.sqrt(bc2, dtype=np.float32))


def _om(v):
    """fl(1.f - v) of the fp32 v"""
    return float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(v, dtype=torch.float32))


def _opt_grad(p, g, wd, gscale, coef):
    """gi = fl(g gscale), _ex: fl(gi coef) (coef an Interval or None), wd != 0: fmaf(wd, p, gi)"""
    gi = exact(g).mul(exact(f32(gscale), like=g), 1)
    if coef is not None:
        gi = gi.mul(coef, 1)
    if f32(wd) != 0.0:
        gi = exact(f32(wd), like=g).fma(exact(p), gi)
    return gi


def adam_intervals(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, coef=None):
    """Brackets of k_adam's (p, m, v) after ONE launch from the given state, one fp32 rounding per operation of the source in its
    uncontracted form (a contracted `pi - (lr/bc1) (mi/denom)` rounds once less and lies inside): gi as _opt_grad;
    mi = fmaf(b1, m, fl(fl(1-b1) gi)); vi = fmaf(b2, v, fl(fl(fl(1-b2) gi) gi)); denom = fl(fl(sqrtf(vi) / bc2_sqrt) + eps);
    p = fl(pi - fl(fl(lr/bc1) fl(mi / denom))).  sqrtf and / are IEEE (correctly rounded, monotone: no fast-math in the build);
    bc1, bc2_sqrt, lr/bc1, 1-b1, 1-b2 are the host's / the kernel's own fp32 scalars, bit for bit.  The brackets of mi and denom
    are propagated as if independent (a superset)."""
    b1, b2, eps, lr = f32(b1), f32(b2), f32(eps), f32(lr)
    bc1, bc2s = adam_bias(b1, b2, step)
    step_size = float(torch.tensor(lr, dtype=torch.float32) / torch.tensor(bc1, dtype=torch.float32))
    s = lambda c: exact(c, like=g)
    gi = _opt_grad(p, g, wd, gscale, coef)
    mi = s(b1).fma(exact(m), s(_om(b1)).mul(gi, 1))
    vi = s(b2).fma(exact(v), s(_om(b2)).mul(gi, 1).mul(gi, 1))
    vi = Interval(vi.lo.clamp_min(0.0), vi.hi)
    den = vi.sqrt().div(s(bc2s), 1).add(s(eps), 1)
    pn = exact(p).add(s(step_size).mul(mi.div(den, 1), 1), 1, -1.0)
    return dict(p=pn, m=mi, v=vi)


def rmsprop_intervals(p, g, sq, buf, lr, alpha, eps, wd, momentum, gscale, coef=None):
    """k_rmsprop, as adam_intervals: s = fmaf(alpha, sq, fl(fl(fl(1-alpha) gi) gi)); avg = fl(sqrtf(s) + eps);
    momentum > 0: b = fmaf(momentum, buf, fl(gi / avg)), p = fl(pi - fl(lr b)); else p = fl(pi - fl(lr fl(gi / avg)))"""
    lr, alpha, eps, momentum = f32(lr), f32(alpha), f32(eps), f32(momentum)
    s = lambda c: exact(c, like=g)
    gi = _opt_grad(p, g, wd, gscale, coef)
    si = s(alpha).fma(exact(sq), s(_om(alpha)).mul(gi, 1).mul(gi, 1))
    si = Interval(si.lo.clamp_min(0.0), si.hi)
    avg = si.sqrt().add(s(eps), 1)
    r = gi.div(avg, 1)
    out = dict(sq=si)
    if momentum > 0:
        r = s(momentum).fma(exact(buf), r)
        out["buf"] = r
    out["p"] = exact(p).add(s(lr).mul(r, 1), 1, -1.0)
    return out


def sgd_intervals(p, g, buf, lr, momentum, dampening, wd, nesterov, step, gscale, coef=None):
    """k_sgd: momentum != 0: b = gi on the first step, else fmaf(momentum, buf, fl(fl(1-dampening) gi)); nesterov:
    gi = fmaf(momentum, b, gi), else b; p = fl(pi - fl(lr gi))"""
    lr, momentum, dampening = f32(lr), f32(momentum), f32(dampening)
    s = lambda c: exact(c, like=g)
    gi = _opt_grad(p, g, wd, gscale, coef)
    out = {}
    if momentum != 0.0:
        b = gi if step == 1 else s(momentum).fma(exact(buf), s(_om(dampening)).mul(gi, 1))
        out["buf"] = b
        gi = s(momentum).fma(b, gi) if nesterov else b
    out["p"] = exact(p).add(s(lr).mul(gi, 1), 1, -1.0)
    return out


def opt_coef_interval(partial, max_norm, like):
    """(norm, coef, Interval of coef) from the fp64 partial table handed to a *_step_ex launch, by tests/gradclip_ref.py: the
    tests' tables hold a few values whose sum is exact in any order, so norm is the one fp32 rounding of the fp64 root; the
    clip's fp32 division is taken at one ulp (it is IEEE in this build; the stats block's last_coef is compared separately)"""
    import numpy as np
    import gradclip_ref as R
    norm = np.float32(np.sqrt(np.float64(sum(partial))))
    c = R.coef(norm, max_norm)
    cv = float(c)
    if cv != cv:
        return norm, c, None
    iv = exact(cv, like=like) if cv == 1.0 else Interval(*(torch.tensor(v, dtype=torch.float64, device=like.device)
                                                         for v in (cv * (1 - 2 * U32), cv * (1 + 2 * U32))))
    return norm, c, iv


def check_ema(ema_dev, d, ema_prev, p_dev, what, family="optimizers"):
    """the EMA behind p: gradclip_ref.ema_bound around the p the device stored"""
    import gradclip_ref as R
    want, bound = R.ema_bound(d, ema_prev.cpu().numpy(), p_dev.cpu().numpy())
    return _assert_bound(ema_dev.cpu(), torch.from_numpy(want), torch.from_numpy(bound) + TINY32, what, family)


_OPT_BUFS = {"adam": ("p", "g", "m", "v"), "rmsprop": ("p", "g", "v", "buf"), "sgd": ("p", "g", "buf")}


def opt_case(kind, st, a, offset, ex=None, family="optimizers"):
    """ONE launch of mnas_<kind>_step (ex None) or mnas_<kind>_step_ex from the state st (cpu fp32 tensors p, g, m, v, buf, ema),
    every buffer a guarded view at element `offset`; a: the keyword arguments of <kind>_intervals.  ex: dict(partial=[fp64 values
    whose sum is exact], max_norm, skip, ema (bool), decay).  Every output inside its bracket, g (and an unused momentum buffer)
    bitwise untouched, canaries on both sides intact; _ex: the EMA inside gradclip_ref.ema_bound around the p the device stored,
    the stats block as documented, a skipped step leaves every buffer bitwise untouched.  -> worst error / bracket."""
    import numpy as np
    lib = L.load()
    names = _OPT_BUFS[kind] + (("ema",) if ex is not None and ex["ema"] else ())
    n = st["p"].numel()
    buf, chk = {}, {}
    for k in names:
        buf[k], chk[k] = guarded((n,), torch.float32, offset=offset)
        buf[k].copy_(st[k])
    before = {k: v.clone() for k, v in buf.items()}
    P = lambda k: buf[k].data_ptr()
    tail, sfx = [], ""
    if ex is not None:
        partial = torch.tensor(ex["partial"], dtype=torch.float64, device="cuda")
        stats = torch.zeros(4, dtype=torch.int64, device="cuda")
        e = L.MnasOptExtra(partial=partial.data_ptr(), nparts=len(ex["partial"]), max_norm=ex["max_norm"], skip_nonfinite=ex["skip"],
                           ema=P("ema") if ex["ema"] else None, ema_decay=ex["decay"], stats=stats.data_ptr(), update_stats=1)
        tail, sfx = [C.byref(e)], "_ex"
    fn = getattr(lib, "mnas_%s_step%s" % (kind, sfx))
    if kind == "adam":
        rc = fn(P("p"), P("g"), P("m"), P("v"), n, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["step"], a["gscale"], *tail, L.cur_stream())
    elif kind == "rmsprop":
        rc = fn(P("p"), P("g"), P("v"), P("buf"), n, a["lr"], a["alpha"], a["eps"], a["wd"], a["momentum"], a["gscale"], *tail, L.cur_stream())
    else:
        rc = fn(P("p"), P("g"), P("buf"), n, a["lr"], a["momentum"], a["dampening"], a["wd"], a["nesterov"], a["step"], a["gscale"],
                *tail, L.cur_stream())
    L.check(rc, kind)
    what = "%s%s n %d offset %d %r" % (kind, sfx, n, offset, a)
    for k in names:
        chk[k](what + " " + k)
    bits_equal(buf["g"], before["g"], what + " g")
    coef = None
    if ex is not None:
        norm, c, coef = opt_coef_interval(ex["partial"], ex["max_norm"], before["p"])
        raw = L.MnasGradStats()
        host = stats.cpu()
        C.memmove(C.byref(raw), host.data_ptr(), 32)
        skipped = bool(ex["skip"]) and not np.isfinite(norm)
        assert raw.steps == 1 and raw.skipped_steps == int(skipped), what
        if np.isfinite(norm):
            assert abs(raw.last_norm - float(norm)) <= 2.0 ** -23 * float(norm), what
            assert abs(raw.last_coef - float(c)) <= 2.0 ** -22 * float(c) and (raw.last_coef == 1.0) == (float(c) == 1.0), what
            assert raw.clipped_steps == int(float(c) < 1.0), what
        else:
            assert not np.isfinite(raw.last_norm), what
        if skipped:
            for k in names:
                bits_equal(buf[k], before[k], what + " skipped step, " + k)
            return 0.0
    b = before
    if kind == "adam":
        ivs = adam_intervals(b["p"], b["g"], b["m"], b["v"], coef=coef, **a)
    elif kind == "rmsprop":
        ivs = rmsprop_intervals(b["p"], b["g"], b["v"], b["buf"], coef=coef, **a)
        ivs["v"] = ivs.pop("sq")
    else:
        ivs = sgd_intervals(b["p"], b["g"], b["buf"], coef=coef, **a)
    worst = 0.0
    for k in _OPT_BUFS[kind]:
        if k in ivs:
            worst = max(worst, check_interval(buf[k], ivs[k], what + " " + k, family))
        else:
            bits_equal(buf[k], before[k], what + " " + k + " (not an output)")
    if ex is not None and ex["ema"]:
        worst = max(worst, check_ema(buf["ema"], ex["decay"], before["ema"], buf["p"], what + " ema", family))
    return worst
