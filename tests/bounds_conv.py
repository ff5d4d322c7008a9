"""Per-element bounds for the conv launches: plain-operand GEMMs, launches whose operand is formed on load, the depthwise sweeps
and the fp32 sums (weight gradients, BatchNorm statistics, the fused reduce).  The operand's interval (intervals.py) is carried
through the fp64 reference (refs64.py) as `slack`."""
import torch

from gpu_util import bf16r
from intervals import SHARES, U32, Interval, _assert_bound, check_sum_bound, to_bf16
from refs64 import f64, ref_dense_dgrad, ref_dense_fwd, ref_dense_wgrad, ref_dw_dgrad, ref_dw_fwd, ref_dw_wgrad

HINGE = 1e-3            # inputs are moved off the ReLU hinge |s*v+t| < HINGE: host and device then agree on every mask bit
MAX_ACT_SPLIT = 1e-3    # largest share of bf16 activation operand elements whose interval straddles a bf16 rounding boundary
MAX_DY_SPLIT = 2e-2     # the same for a dy operand (it cancels: three terms of either sign)
MAX_HINGE_MOVED = 1e-2  # largest share of elements off_hinge may move


def check_gemm_bound(hip, ref, S, K, what):
    """Per-element bound for a GEMM launch whose operands need no transform on load (plain activation, materialised dy).
    hip: the bf16 output; ref: the fp64 result over the same bf16 operands; S = |bias| + sum |a|*|w| (the same reference on
    absolute values); K: reduction length.  Derivation: a product of two bf16 numbers is exact in fp32; each of the K
    accumulations (and the bias add) loses at most 2^-23 relative to the running magnitude <= S, rounding toward zero
    included, so the fp32 result is within (K+1)*2^-23*S of ref; the bf16 store (round to nearest even, 8 significand bits)
    adds at most half an ulp, which is at most 2^-8*|value| (reached just above a power of two; 2^-9 just below one).
    Asserted for EVERY element: |hip - ref| <= 2^-8*|ref| + (K+1)*2^-22*S -- the store term is the exact worst case, the
    accumulation term carries a factor of two (it also absorbs a value that the fp32 error moves across a rounding
    boundary or a power of two).  Correct kernels were measured at up to 0.99 of this bound.  An operand formed on load
    (act-on-load, dy-on-load) is outside this derivation: check_onload_bound below is this bound plus the operand's
    interval.  The squeeze-excite kernels and the gated act-on-load (act8g), the stem's weight and input gradients,
    mnas_add_act / the pooling glue and the finalizes have their own helpers in bounds_se.py."""
    assert hip.shape == ref.shape == S.shape, (what, hip.shape, ref.shape, S.shape)
    return _assert_bound(hip, ref, 2.0 ** -8 * ref.double().abs() + (K + 1) * 2.0 ** -22 * S.double(), what, None)


def _pre(v, s, t):
    return s.double().to(v.device) * v.double() + t.double().to(v.device)


def _on_hinge(v, s, t):
    """|s*v+t| < HINGE, except where v == 0 and t == 0: there s*v+t is exactly zero in fp32 and in fp64 alike"""
    exact0 = (v.double() == 0) & (t.double().to(v.device) == 0).expand_as(v)
    return (_pre(v, s, t).abs() < HINGE) & ~exact0


def _hinge_share(bad, verb):
    share = float(bad.double().mean())
    assert share <= MAX_HINGE_MOVED, "%s %.3g of the elements (limit %.3g)" % (verb, share, MAX_HINGE_MOVED)
    SHARES["hinge"] = max(SHARES.get("hinge", 0.0), share)


def off_hinge(v, s, t):
    """v (..., C) fp32 holding bf16 values; s, t [C]: move the elements with |s*v+t| < HINGE to where s*v+t ~ +0.05 (bf16).
    An element with v == 0 under t == 0 stays: its s*v+t is the exact zero on host and device.  At most MAX_HINGE_MOVED of the
    elements may need moving (a test whose inputs sit on the hinge wholesale is testing something else)."""
    sd, td = s.double().to(v.device), t.double().to(v.device)
    bad = _on_hinge(v, s, t)
    _hinge_share(bad, "off_hinge would move")
    alt = bf16r(((0.05 - td) / sd).float()).expand_as(v)
    out = torch.where(bad, alt, v)
    assert not bool(_on_hinge(out, s, t).any())
    return out


def zero_on_hinge(g, y, s, t):
    """Where y cannot be moved (it is another kernel's output, e.g. the forward's stored y that RECOMP recomputes): g = 0 at the
    elements with y on the hinge, so that g*[s*y+t > 0] = 0 whichever way the mask bit falls.  Same share limit as off_hinge."""
    bad = _on_hinge(y, s, t)
    _hinge_share(bad, "zero_on_hinge would clear")
    return torch.where(bad, torch.zeros_like(g), g)


def relu_mask(v, s, t):
    """[s*v+t > 0] in fp64; v must be off the hinge (off_hinge), so the device's fp32 fma (within u*|s*v+t|) gives the same bits"""
    assert not bool(_on_hinge(v, s, t).any()), "mask input on the ReLU hinge: move it with off_hinge first"
    return _pre(v, s, t) > 0


def act_interval(z, s, t, bf16, device="cpu"):
    """Interval of the act-on-load operand relu(s*z+t) over the last (channel) dimension; z holds bf16 values, s, t fp32.
    Exact value pre = s*z+t (fp64).  The device evaluates one fmaf (act8, dw_act_raw: within u*|pre| <= u*(|s||z|+|t|)); an
    unfused evaluation rounds the product and the sum (within 2u*(|s||z|+|t|) to first order), so eps = 2u*(|s||z|+|t|) covers
    both.  relu is monotone: an fp32 operand (the depthwise sweeps) lies in [relu(pre-eps), relu(pre+eps)].  bf16=True: the MFMA
    kernels round it to bf16 (pack_bf16, round to nearest even), which is monotone too: [bf16(relu(pre-eps)), bf16(relu(pre+eps))].
    Asserted: at most MAX_ACT_SPLIT of the bf16 elements have lo != hi (the interval straddles a rounding boundary).
    .D = |s||z|+|t|, the magnitude the depthwise bound's S is built from."""
    z, s, t = f64(z, device), f64(s, device), f64(t, device)
    pre = s * z + t
    D = s.abs() * z.abs() + t.abs()
    eps = 2 * U32 * D
    iv = Interval(torch.relu(pre - eps), torch.relu(pre + eps), D, torch.relu(pre))
    return to_bf16(iv, MAX_ACT_SPLIT, "act") if bf16 else iv


def dy_interval(g, y, coef, bf16, device="cpu", g_masked=False):
    """Interval of the dy-on-load operand dy = c1*g*[s*y+t > 0] + c2*y + c3 (coef rows 0..4) over the last dimension; g, y hold
    bf16 values.  y must be off the ReLU hinge (asserted; an element with g == 0 is exempt: its dz is 0 under either mask bit), so
    the mask bit is the device's.  With D = |c1||g| +
    |c2||y| + |c3|: dy8 / dw_read_dy evaluate fma(c1, dz, fma(c2, y, c3)) -- two nested roundings, within 2u*D -- and an unfused
    evaluation twice as many: eps = 4u*D.  fp32 operand (depthwise): [dy-eps, dy+eps]; bf16=True (pack8 of dy8 in the MFMA
    kernels): both ends rounded to bf16.  Asserted: at most MAX_DY_SPLIT of the bf16 elements have lo != hi.
    g_masked: g already holds g*mask (the g_masked form of mnas_dw_bwd), no mask is applied."""
    g, y, cf = f64(g, device), f64(y, device), f64(coef, device)
    s, t, c1, c2, c3 = cf[0], cf[1], cf[2], cf[3], cf[4]
    if not g_masked:
        assert not bool((_on_hinge(y, s, t) & (g != 0)).any()), "dy-on-load: y on the ReLU hinge under a non-zero g (off_hinge / zero_on_hinge)"
    dz = g if g_masked else g * (s * y + t > 0)
    d = c1 * dz + c2 * y + c3
    D = c1.abs() * g.abs() + c2.abs() * y.abs() + c3.abs()
    eps = 4 * U32 * D
    iv = Interval(d - eps, d + eps, D, d)
    return to_bf16(iv, MAX_DY_SPLIT, "dy") if bf16 else iv


def onload_elem_err(slack, S, K):
    """what the fp32 value in the accumulator (before the bf16 store) may differ from the fp64 reference by: (K+1)*2^-22*S + slack"""
    return (K + 1) * 2.0 ** -22 * S.double() + slack.double()


def check_onload_bound(hip, ref, slack, S, K, what, family="mfma on-load"):
    """Per-element bound for an MFMA launch (bf16 output) whose operand is formed on load and known as an Interval `a` (bf16 ends).
    ref = conv(a.mid, w) (+bias, +resid); slack = conv(a.half, |w|): how far the exact result over ANY operand inside the
    interval can lie from ref; S = conv(a.amax, |w|) + |bias| + |resid|.  As check_gemm_bound: bf16 x bf16 products are exact,
    K accumulations and the bias / residual add lose (K+1)*2^-23*S, doubled; the bf16 store rounds a value of at most
    |ref|+slack (+ the fp32 error, which the doubled accumulation term absorbs) by at most 2^-8 of it.  EVERY element:
        |hip - ref| <= 2^-8*(|ref| + slack) + (K+1)*2^-22*S + slack.
    With lo == hi everywhere (slack = 0) this is check_gemm_bound."""
    bound = 2.0 ** -8 * (ref.double().abs() + slack.double()) + onload_elem_err(slack, S, K)
    return _assert_bound(hip, ref, bound, what, family)


def dw_elem_err(S, k):
    """fp32 error of a depthwise accumulator before its bf16 store: (2k^2+2)*2^-23*S"""
    return (2 * k * k + 2) * 2.0 ** -23 * S.double()


def check_dw_bound(hip, ref, S, k, what, family="depthwise"):
    """Per-element bound for the depthwise sweeps (fp32 operands formed on read, fp32 weights as given -- NOT rounded to bf16 by
    the test --, k*k taps accumulated in fp32, bf16 output).  ref: the fp64 result over the exact operands (relu(s*z+t) resp. dy in
    fp64).  S: the same sum over magnitudes -- forward |bias| + sum (|s||z|+|t|)*|w| (act_interval(...).D), input gradient
    sum D*|w| (dy_interval(...).D).  Each tap is one fma rounding (or a multiply and an add rounding), 2^-24 of a running
    magnitude <= S each: at most 2k^2*2^-24*S; the operand's own rounding (u resp. 2u of its magnitude, act_interval /
    dy_interval) is at most 2*2^-24*S more; doubled as in check_gemm_bound: (2k^2+2)*2^-23*S.  The bf16 store adds 2^-8*|value|.
        |hip - ref| <= 2^-8*|ref| + (2k^2+2)*2^-23*S      for EVERY element."""
    bound = 2.0 ** -8 * ref.double().abs() + dw_elem_err(S, k)
    return _assert_bound(hip, ref, bound, what, family)


def stats_bound_terms(ref, e, dims=None):
    """BatchNorm statistics of an fp32 accumulator v with |v - ref| <= e element by element (the kernels sum the accumulator, not
    the stored bf16 value: mnas_stat2 / `s1 += v; s2 = fma(v, v, s2)` sit before pack_bf16 in every forward epilogue).  Returns
    (ref1, S1, slack1, ref2, S2, slack2) per channel for check_sum_bound: sum v against sum ref with slack sum e; sum v^2 against
    sum ref^2 with slack sum (2|ref|e + e^2); S over (|ref|+e) resp. its square."""
    ref, e = ref.double(), e.double()
    dims = tuple(range(ref.dim() - 1)) if dims is None else dims
    a = ref.abs() + e
    return (ref.sum(dims), a.sum(dims), e.sum(dims), (ref * ref).sum(dims), (a * a).sum(dims), (2 * ref.abs() * e + e * e).sum(dims))


def check_stats_bound(st, ref, e, M, what, family="statistics"):
    """st: the [2][C][P] table of a forward launch; ref (..., C): fp64 reference elements; e: their fp32 error bound.  c = 1 for
    sum v, c = 2 for sum v^2 (the square is rounded)."""
    P = st.shape[-1]
    p = st.double().sum(-1)
    r1, S1, k1, r2, S2, k2 = stats_bound_terms(ref, e)
    a = check_sum_bound(p[0].to(r1.device), r1, S1, M, P, 1, what + " stats sum", k1, family)
    b = check_sum_bound(p[1].to(r1.device), r2, S2, M, P, 2, what + " stats sum of squares", k2, family)
    return max(a, b)


def check_red_bound(table, gq, yin, bn, M, what, family="fused reduce"):
    """Fused BatchNorm-backward reduce (sum dz, sum dz*xhat) per channel; table [2][C][P].  The kernels sum the gradient AS STORED
    (mnas_red2 takes the packed bf16 pair; dw: f2bf(pk)): gq is the launch's own bf16 output, yin the raw output of the producer
    (off the hinge), bn its bnbuf.  dz = gq*[s*y+t>0] is exact: c = 1 for sum dz.  xhat = fma(y, inv, m) with m = -mean*inv
    rounded, within 2u*(|y|+|mean|)*|inv| of (y-mean)*inv: c = 2 for sum dz*xhat with S = sum |dz|*(|y|+|mean|)*|inv|."""
    C_ = gq.shape[-1]
    gq, yin = gq.reshape(-1, C_), yin.reshape(-1, C_)
    bn = bn.double().to(gq.device)
    acc = [torch.zeros(C_, dtype=torch.float64, device=gq.device) for _ in range(4)]
    step = max(1, (8 << 20) // C_)                       # fp64 temporaries of at most 8 M elements
    for m0 in range(0, gq.shape[0], step):
        g, y = gq[m0:m0 + step].double(), yin[m0:m0 + step].double()
        dz = g * relu_mask(y, bn[0], bn[1])
        xhat = (y - bn[5]) * bn[6]
        xabs = (y.abs() + bn[5].abs()) * bn[6].abs()
        for a_, v in zip(acc, (dz, dz.abs(), dz * xhat, dz.abs() * xabs)):
            a_ += v.sum(0)
    P = table.shape[-1]
    p = table.double().sum(-1).to(gq.device)
    a = check_sum_bound(p[0], acc[0], acc[1], M, P, 1, what + " sum dz", None, family)
    b = check_sum_bound(p[1], acc[2], acc[3], M, P, 2, what + " sum dz*xhat", None, family)
    return max(a, b)


def prod_slack(a, b):
    """element-wise slack of a product of two interval operands: |a.mid|*b.half + |b.mid|*a.half + a.half*b.half"""
    return a.mid.abs() * b.half + b.mid.abs() * a.half + a.half * b.half


def onload_fwd_terms(a, w, bias=None, stride=1, pad=None, device="cpu"):
    """(ref, slack, S) of check_onload_bound for a forward conv over the interval operand a (N,H,W,Ci), w (Co,Ci,k,k)"""
    aw = f64(w, device).abs()
    ref = ref_dense_fwd(a.mid, w, bias, stride, pad, device)
    slack = ref_dense_fwd(a.half, aw, None, stride, pad, device)
    S = ref_dense_fwd(a.amax, aw, None if bias is None else bias.abs(), stride, pad, device)
    return ref, slack, S


def onload_dgrad_terms(d, w, H, W, stride=1, pad=None, resid=None, device="cpu"):
    """(ref, slack, S) of check_onload_bound for an input gradient over the interval operand d (N,Ho,Wo,Co), w (Co,Ci,k,k)"""
    aw = f64(w, device).abs()
    ref = ref_dense_dgrad(d.mid, w, H, W, stride, pad, device)
    slack = ref_dense_dgrad(d.half, aw, H, W, stride, pad, device)
    S = ref_dense_dgrad(d.amax, aw, H, W, stride, pad, device)
    if resid is not None:
        r = f64(resid, device)
        ref, S = ref + r, S + r.abs()
    return ref, slack, S


def _sum_terms(wgrad, a, d, *args):
    """(ref, S, slack) of a weight gradient `wgrad` over two interval operands"""
    ref = wgrad(a.mid, d.mid, *args)
    S = wgrad(a.amax, d.amax, *args)
    slack = (S - wgrad(a.mid.abs(), d.mid.abs(), *args)).clamp_min(0)
    return ref, S, slack


def wgrad_terms(a, d, k, stride=1, pad=None, device="cpu"):
    """(ref, S, slack) of check_sum_bound for a dense weight gradient over interval operands a (N,H,W,Ci), d (N,Ho,Wo,Co)
    -> (Co,Ci,k,k).  slack = sum prod_slack = S - sum |a.mid||d.mid|, because amax = |mid| + half for any interval (exactly zero
    for two zero-width intervals: both sums are then the same computation)."""
    return _sum_terms(ref_dense_wgrad, a, d, k, stride, pad, device)


def dw_fwd_terms(a, w, bias=None, stride=1, device="cpu"):
    """(ref, S) of check_dw_bound for the depthwise forward over the fp32 interval operand a = act_interval(..., bf16=False) (or
    Interval.exact of a plain input): ref over the exact operand a.val, S = |bias| + sum a.D*|w|"""
    aw = f64(w, device).abs()
    ref = ref_dw_fwd(a.val, w, bias, stride, device)
    S = ref_dw_fwd(a.D, aw, None if bias is None else bias.abs(), stride, device)
    return ref, S


def dw_dgrad_terms(d, w, H, W, stride=1, device="cpu"):
    """(ref, S) of check_dw_bound for the depthwise input gradient over d = dy_interval(..., bf16=False): S = sum D*|w|"""
    aw = f64(w, device).abs()
    return ref_dw_dgrad(d.val, w, H, W, stride, device), ref_dw_dgrad(d.D, aw, H, W, stride, device)


def dw_wgrad_terms(a, d, k, stride=1, device="cpu"):
    """(ref, S, slack) of check_sum_bound (c = 2) for the depthwise weight gradient over fp32 interval operands (slack as in
    wgrad_terms)"""
    return _sum_terms(ref_dw_wgrad, a, d, k, stride, device)
