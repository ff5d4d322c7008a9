"""Per-element bounds for squeeze-excite, the stem gradients, the glue kernels and the BatchNorm finalizes, in the conventions
of intervals.py."""
import torch

from bounds_conv import MAX_ACT_SPLIT, act_interval
from gpu_util import bf16r
from intervals import D64, U32, WORST, Interval, check_interval, hull, store32, sum_bound, sum_interval, to_bf16, widen
from refs64 import f64, ref_dense_dgrad


def sigmoid_interval(v, device=None):
    """Bracket of se_sigmoid(v) = 1.f / (1.f + __expf(-v)) (csrc/mnas_se.hip) around the fp64 sigmoid s; v fp32 as the device reads it.
    __expf(x) is the hardware 2^t of t = fl(x * fl(log2 e)).  With e = exp(-v):
      the constant fl(log2 e) and the product each move t by at most u|t|, i.e. 2^t by a factor within 2|t| ln2 u = 2|v| u of 1;
      the hardware exponential is taken at its documented accuracy of one ulp = 2u relative -- the ONE assumption here that IEEE 754
      does not give; the mnas_se_gate sweep of tests/test_gpu_se.py checks it directly;
      the add 1.f + e and the division (IEEE: the build has no fast-math) are within u each;
      an error of e reaches s = 1/(1+e) with the factor e/(1+e) <= 1.
    To first order (2|v| + 4)u; (2|v| + 6)u leaves room for every second-order term at |v| <= 2^10:
        |se_sigmoid(v) - s| <= (2|v| + 6) u s + 2^-126     (the floor: a subnormal quotient, an exponential flushed to zero)
    and the quotient of 1 by a number >= 1 lies in [0, 1]."""
    v = v.double() if device is None else f64(v, device)
    s = torch.sigmoid(v)
    r = (2 * v.abs() + 6) * U32 * s + 2.0 ** -126
    return Interval((s - r).clamp_min(0.0), (s + r).clamp_max(1.0), s, s)


def check_sigmoid(got, v, what, family="se_sigmoid"):
    """got = se_sigmoid(v) from the device: inside sigmoid_interval(v); returns (and keeps in WORST) the largest
    |got - s| / ((2|v| + 6) u s + 2^-126), the error against the bracket's half width BEFORE its ends are clamped to [0, 1]"""
    iv = sigmoid_interval(v)
    check_interval(got, iv, what, None)
    r = float(((got.double().cpu() - iv.val).abs() / ((2 * v.double().abs() + 6) * U32 * iv.val + 2.0 ** -126)).max())
    if family:
        WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def sig1m_interval(v, device=None):
    """Bracket of fl(sg * fl(1.f - sg)), sg = se_sigmoid(v): g(x) = x(1-x) over the bracket [l, h] of sg -- g rises up to 1/2 and
    falls after it, so its range is [min(g(l), g(h)), max(g(l), g(h))], or up to 1/4 where l <= 1/2 <= h -- widened by the two
    roundings (the subtraction, the product).  Not linearised: 1 - sg cancels for large v, and the bracket of sg is then a large
    share of it."""
    sg = sigmoid_interval(v, device)
    gl, gh = sg.lo * (1 - sg.lo), sg.hi * (1 - sg.hi)
    lo, hi = torch.minimum(gl, gh), torch.maximum(gl, gh)
    hi = torch.where((sg.lo <= 0.5) & (sg.hi >= 0.5), torch.full_like(hi, 0.25), hi)
    lo, hi = widen(lo, hi, 2)
    return Interval(lo, hi, None, sg.val * (1 - sg.val))


def gate_nhwc(gate, shape):
    """(N, C) gate Interval -> broadcastable against (N, H, W, C)"""
    N, C_ = gate.lo.shape
    view = (N,) + (1,) * (len(shape) - 2) + (C_,)
    return Interval(gate.lo.view(view), gate.hi.view(view), None, None if gate.val is None else gate.val.view(view))


def gated_act_interval(z, s, t, gate, bf16, device="cpu"):
    """Interval of the gated operand fl(a * sg): a = relu(fma(z, s, t)) (s, t None: a = z, exact) and sg the gate of the element's
    (image, channel), an Interval >= 0 (sigmoid_interval) broadcastable against z -- what act8g (MnasConvGemm.gate) and k_se_scale
    form: ONE more fp32 rounding after act_interval's value.  Both factors' brackets are >= 0 under the activation, so the product
    lies in [lo*glo*(1-u), hi*ghi*(1+u)]; a plain (signed) a takes the hull of the corner products.  bf16=True: both ends rounded
    to bf16 (pack8), and at most MAX_ACT_SPLIT of the elements may straddle a rounding boundary, as for act_interval."""
    if s is None:
        a = Interval.exact(z, device)
    else:
        a = act_interval(z, s, t, False, device)
    g = Interval(f64(gate.lo, device), f64(gate.hi, device))
    p = a.mul(g, 1)
    gv = f64(gate.val, device) if gate.val is not None else (g.lo + g.hi) / 2
    iv = Interval(p.lo, p.hi, a.D * g.hi, a.val * gv)
    return to_bf16(iv, MAX_ACT_SPLIT, "gated act") if bf16 else iv


def se_apply_interval(gq, u, dz, HW, device="cpu"):
    """k_se_bwd_apply's fp32 value fma(gq, sg, zz) per element, gq (N,H,W,C) bf16 values, u, dz (N,C): sg in sigmoid_interval(u);
    zz = fl(dz * fl(1/HW)): the reciprocal within u, the product within u more; the fma rounds the exact gq*sg + zz once, an
    unfused evaluation the product too: within u(|gq| sg + |zz|) either way."""
    gq = f64(gq, device)
    sg = gate_nhwc(sigmoid_interval(u, device), gq.shape)
    inv = 1.0 / HW
    zz = gate_nhwc(Interval.exact(dz, device).mul(Interval(torch.full((), inv * (1 - U32), dtype=torch.float64, device=device),
                                                           torch.full((), inv * (1 + U32), dtype=torch.float64, device=device)), 1), gq.shape)
    p = Interval.exact(gq).mul(sg, 0)
    r = U32 * (p.amax + zz.amax) * (1 + U32)
    return Interval(p.lo + zz.lo - r, p.hi + zz.hi + r)


def se_reduce_terms(gs, a, HW):
    """(ref, S, slack) per (image, channel) of sum_hw gs*a for mnas_se_bwd_reduce: gs (N,H,W,C) exact bf16 values, a the fp32
    operand Interval (act_interval(..., bf16=False), or Interval.exact for a plain input).  One fma per pixel (c = 1)."""
    g = gs.double().to(a.lo.device)
    N, C_ = g.shape[0], g.shape[-1]
    f = lambda t: t.reshape(N, HW, C_).sum(1)
    return f(g * a.mid), f(g.abs() * a.amax), f(g.abs() * a.half)


def se_geom(N, HW, C_):
    """(G, R, chunk, splits) as csrc/mnas_se.hip::se_geom derives them; the tests assert it against mnas_se_scratch_bytes /
    mnas_se_bwd_apply_cols"""
    G_ = C_ // 8
    R = 256 // G_
    sp = max(1, min(2048 // N, (HW + 4 * R - 1) // (4 * R)))
    chunk = ((HW + sp - 1) // sp + R - 1) // R * R
    return G_, R, chunk, (HW + chunk - 1) // chunk


def se_proj_finalize_intervals(wp, N, kseg, W, u, dW0=None):
    """mnas_se_proj_finalize from the wpartial table the segment-mode mnas_pw_bwd wrote (read BEFORE the finalize: it folds in
    place): wp (N*kseg, Co, Ci) fp32, W (Co, Ci) the fp32 master weight, u (N, Ci).  p[n] = sum_j wp[n*kseg+j] in fp32.
      du[n][c] = fl(fl(acc * sg) * fl(1 - sg)), acc = sum_o fma(W, p, acc): Co*kseg terms, the term p itself rounded (c = 2), the
        256/Ci output-channel groups met in LDS (P); then the sig1m bracket and one more rounding.
      dW[o][c] (+)= sum_n fl(p[n] * sg[n]): N*kseg terms, c = 2, sg's bracket in the slack; the accumulate add is check_sum_bound's +1.
    Returns (du Interval, dW ref, dW S, dW slack, M of dW)."""
    dev = wp.device
    Co, Ci = W.shape
    p = wp.double().view(N, kseg, Co, Ci)
    pa = p.abs().sum(1)
    p = p.sum(1)
    W = f64(W, dev)
    G_ = 256 // Ci if Ci <= 256 else 0
    acc = sum_interval((W * p).sum(1), (W.abs() * pa).sum(1), Co * kseg, G_, 2)
    du = acc.mul(sig1m_interval(u, dev), 1)
    sg = sigmoid_interval(u, dev)
    sl, sh = sg.lo.view(N, 1, Ci), sg.hi.view(N, 1, Ci)
    ref, S, slack = (p * (sl + sh) / 2).sum(0), (pa * sh).sum(0), (pa * (sh - sl) / 2).sum(0)
    if dW0 is not None:
        ref, S = ref + f64(dW0, dev), S + f64(dW0, dev).abs()
    return du, ref, S, slack, N * kseg


def se_fc_fwd_intervals(z, W1, b1, W2, b2):
    """mnas_se_fc_fwd (fp32 dot products, fma or multiply-and-add: c = 2): hb = relu(W1 z + b1) over E terms plus the bias,
    u = W2 hb + b2 over R terms plus the bias with |W2| err(hb) as slack, gate = se_sigmoid(u) over u's bracket (the sigmoid and
    both ends of its bracket rise with v for |v| < 16, asserted).  Returns (hb, u, gate) Intervals (N,R), (N,E), (N,E)."""
    z, W1, b1, W2, b2 = (t.double() for t in (z, W1, b1, W2, b2))
    E, R = W2.shape
    pre = sum_interval(z @ W1.t() + b1, z.abs() @ W1.abs().t() + b1.abs(), E, 1, 2)
    hb = Interval(torch.relu(pre.lo), torch.relu(pre.hi))
    u = sum_interval(hb.mid @ W2.t() + b2, hb.amax @ W2.abs().t() + b2.abs(), R, 1, 2, hb.half @ W2.abs().t())
    assert float(u.amax.max()) < 16
    gate = Interval(sigmoid_interval(u.lo).lo, sigmoid_interval(u.hi).hi)
    return hb, u, gate


def se_fc_bwd_terms(du, z, hb_dev, W1, W2, base=None):
    """mnas_se_fc_bwd against fp64, every product c = 2.  hb_dev: the hidden row the device stored (the mask and dW2's operand are
    the device's own values).  dh = (du W2)[hb_dev > 0]: E terms, 256/(2R) row slices (P); dz = dh W1: R terms over dh's bracket;
    dW1 / db1 / dW2 / db2: N terms in 16 image phases (P = 16), plus the accumulate target `base` (a dict) where given.
    Returns dh, dz Intervals and {name: (ref, S, slack, c)} for check_sum_bound with M = N, P = 16."""
    du, z, hb, W1, W2 = (t.double() for t in (du, z, hb_dev, W1, W2))
    N, E = du.shape
    R = W1.shape[0]
    m = (hb > 0).double()
    dh = sum_interval((du @ W2) * m, (du.abs() @ W2.abs()) * m, E, 256 // (2 * R), 2)
    dz = sum_interval(dh.mid @ W1, dh.amax @ W1.abs(), R, 0, 2, dh.half @ W1.abs())
    t = {"dW1": (dh.mid.t() @ z, dh.amax.t() @ z.abs(), dh.half.t() @ z.abs(), 2),
         "db1": (dh.mid.sum(0), dh.amax.sum(0), dh.half.sum(0), 1),
         "dW2": (du.t() @ hb, du.abs().t() @ hb.abs(), None, 2),
         "db2": (du.sum(0), du.abs().sum(0), None, 1)}
    if base is not None:
        t = {k: (r + base[k].double(), S + base[k].double().abs(), sl, c) for k, (r, S, sl, c) in t.items()}
    return dh, dz, t


def stem_dgrad_terms(d, w, H, W, aff=None, device="cpu"):
    """(ref, bound) of mnas_stem_dgrad's fp32 NCHW result.  d: the bf16 dy Interval (N,Ho,Wo,Co) (dy_interval(..., bf16=True): dy8 and
    pack_bf16 in the kernel); w: the weights AS THE KERNEL ROUNDS THEM, bf16 values (Co,3,3,3).  Every product of two bf16 values is
    exact in fp32 and every term one fmaf: at most K = 4*Co roundings (four contributing output pixels at most) of 2^-24 of a
    running magnitude <= S = sum |dy||w|, doubled as in check_gemm_bound: (K+1)*2^-23*S, plus the slack of the dy brackets.  No bf16
    store.  in_affine: one more product, acc * scale[plane]: the bound times |scale| and u of the scaled result more."""
    aw = f64(w, device).abs()
    Co = w.shape[0]
    ref = ref_dense_dgrad(d.mid, w, H, W, 2, 1, device)
    slack = ref_dense_dgrad(d.half, aw, H, W, 2, 1, device)
    S = ref_dense_dgrad(d.amax, aw, H, W, 2, 1, device)
    bound = (4 * Co + 1) * 2.0 ** -23 * S + slack
    if aff is not None:
        sc = f64(aff[0], device)
        ref, bound = ref * sc, bound * sc.abs()
        bound = bound + U32 * (ref.abs() + bound)
    return ref.permute(0, 3, 1, 2).contiguous(), bound.permute(0, 3, 1, 2).contiguous()


def stem_wgrad_band_rows(W, Wo):
    """output rows per band of k_stem_wgrad: 4, halved while stem_lds (csrc/mnas_stem.hip) exceeds 52 KB"""
    def lds(rb):
        lw = (W + 4 + 1) & ~1
        return 3 * (2 * rb + 1) * lw * 2 + 5 * 32 * 4 + ((rb * Wo + 31) & ~31) * 40 * 2
    rb = 4
    while rb > 1 and lds(rb) > 52 * 1024:
        rb >>= 1
    return rb


def pool_act_terms(a, HW):
    """(ref, bound) of mnas_pool_act: a the fp32 operand Interval (N,HW,C) (act_interval(..., bf16=False) or Interval.exact).  The
    sum of HW terms over R row lanes is check_sum_bound's (c = 1: one add per term; the fma of a virtual operand is in the
    bracket, whose half width is the slack); the division by (float)HW (exact for HW < 2^24, IEEE) rounds once more."""
    C_ = a.lo.shape[-1]
    R = 256 // (C_ // 8)
    b = sum_bound(a.amax.sum(1), HW, R, 1, a.half.sum(1))
    ref = a.mid.sum(1)
    return ref / HW, b / HW + U32 * (ref.abs() + b) / HW


def add_act_interval(A, B=None):
    """fp32 value of mnas_add_act per element: act(a) [+ act(b)] from the operands' fp32 Intervals; the add rounds once more"""
    return A if B is None else Interval(*widen(A.lo + B.lo, A.hi + B.hi, 1))


def partial_sum_interval(p):
    """bn_partial_sums<TPC> (csrc/mnas_elementwise.hip) over the last dimension of the fp32 table p: thread t of TPC (64 up to 256
    partials, 256 above) adds the partials t + 4*TPC*i + TPC*j into fp32 accumulator j, T = ceil(nparts / (4*TPC)) of them each,
    the first onto 0.f: T - 1 roundings of at most u of the accumulator's running magnitude, together (T-1)*u*sum|p| -- zero up to
    256 partials and again from 257 to 1024.  Everything after that is double: D64 of sum|p|."""
    n = p.shape[-1]
    tpc = 64 if n <= 256 else 256
    T = -(-n // (4 * tpc))
    s, a = p.double().sum(-1), p.double().abs().sum(-1)
    d = ((T - 1) * U32 + D64) * a
    return Interval(s - d, s + d)


def bn_fwd_finalize_intervals(partial, count, gamma, beta, rm, rv, momentum, eps):
    """mnas_bn_fwd_finalize (training) from the fp32 table partial [2][C][nparts] exactly as given to the kernel; gamma, beta, rm, rv
    fp32 [C]; momentum, eps as the fp32 values the ABI passes.  Bracketed, not linearised (var = s2/count - mean^2 cancels):
      s1, s2 in partial_sum_interval; mean = s1/count; var = s2/count - mean^2 within ds2/count + 2|mean| dmean + dmean^2 (and D64
      of s2/count + mean^2: the double subtraction cancels too), clamped at 0 at both ends as the kernel clamps;
      invstd = 1/sqrt(var + eps) falls with var; s = gamma invstd, t = beta - mean gamma invstd, running_mean, running_var
      (unbiased: var count/(count-1), var itself at count <= 1) are (bi)linear in (mean, invstd) resp. var: the hull over the corners.
    Each output is then rounded once to fp32.  Returns {name: Interval} for s, t, mean, invstd, running_mean, running_var."""
    s1, s2 = partial_sum_interval(partial[0]), partial_sum_interval(partial[1])
    g, b, rm, rv = gamma.double(), beta.double(), rm.double(), rv.double()
    mom, eps = float(torch.tensor(momentum, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    ml, mh = s1.lo / count, s1.hi / count
    mean, dmean = (ml + mh) / 2, (mh - ml) / 2
    e2 = s2.mid / count
    var = e2 - mean * mean
    dvar = s2.half / count + 2 * mean.abs() * dmean + dmean * dmean + D64 * (e2.abs() + mean * mean)
    vl, vh = (var - dvar).clamp_min(0.0), (var + dvar).clamp_min(0.0)
    il, ih = 1 / torch.sqrt(vh + eps), 1 / torch.sqrt(vl + eps)
    unb = count / (count - 1.0) if count > 1.0 else 1.0
    out = {"mean": store32(ml, mh), "invstd": store32(il, ih)}
    out["s"] = store32(*hull(g * il, g * ih))
    tl, th = hull(*[b - m_ * g * i_ for m_ in (ml, mh) for i_ in (il, ih)])
    out["t"] = store32(tl, th, b.abs() + torch.maximum(ml.abs(), mh.abs()) * g.abs() * ih)
    out["running_mean"] = store32(*hull((1 - mom) * rm + mom * ml, (1 - mom) * rm + mom * mh), (1 - mom) * rm.abs() + mom * torch.maximum(ml.abs(), mh.abs()))
    out["running_var"] = store32((1 - mom) * rv + mom * vl * unb, (1 - mom) * rv + mom * vh * unb)
    return out


def bn_bwd_finalize_intervals(partial, count, bn, dgamma0=None, dbeta0=None, frozen=False, dbias0=None):
    """mnas_bn_bwd_finalize / _frozen from the fp32 table partial [2][C][nparts] (sum dz, sum dz*xhat) and the bnbuf rows s (0),
    mean (5), invstd (6) as given: s1, s2 in partial_sum_interval, then double, one fp32 rounding per output.
      rows 2..4: c1 = s; c2 = -s invstd s2/count; c3 = s (mean invstd s2/count - s1/count): hull over the ends of s1, s2;
      dgamma = dgamma0 + fl(s2), dbeta = dbeta0 + fl(s1) (accumulate: one more fp32 add); frozen: dbias = dbias0 + fl(s s1), rows 2..4 untouched."""
    s1, s2 = partial_sum_interval(partial[0]), partial_sum_interval(partial[1])
    bn = bn.double()
    s, mean, inv = bn[0], bn[5], bn[6]

    def acc(iv, base):
        return iv if base is None else Interval(*widen(iv.lo + base.double(), iv.hi + base.double(), 1))
    out = {"dgamma": acc(store32(s2.lo, s2.hi), dgamma0), "dbeta": acc(store32(s1.lo, s1.hi), dbeta0)}
    if frozen:
        out["dbias"] = acc(store32(*hull(s * s1.lo, s * s1.hi)), dbias0)
        return out
    out["c1"] = Interval(s, s)
    out["c2"] = store32(*hull(-s * inv * s2.lo / count, -s * inv * s2.hi / count))
    c3 = [s * (mean * inv * b_ / count - a_ / count) for a_ in (s1.lo, s1.hi) for b_ in (s2.lo, s2.hi)]
    out["c3"] = store32(*hull(*c3), s.abs() * ((mean * inv).abs() * s2.amax + s1.amax) / count)
    return out


def bn_fwd_partials(u, count):
    """The fp32 table [2][C+3][nparts] of the mnas_bn_fwd_finalize tests from u = uniform(-1, 1) of that shape, built in fp64 and
    rounded ONCE to fp32.  Channels [0, C): mean ~ 0.3*u, var in [0.5, 0.9] (the distribution the test always had).  The last
    three: |mean|/std = 30 (mean 60, var 4), |mean|/std = 300 (mean 600, var 4) -- where var = s2/count - mean^2 cancels 3 resp. 5
    decimal digits -- and a constant channel (every element 1.5) whose sum of squares is rounded DOWN by 2^-20, so that var comes
    out negative and takes the clamp."""
    u = u.double()
    nparts = u.shape[-1]
    per = count / nparts
    mean_p = 0.3 * u[0]
    p = torch.stack([per * mean_p, per * (mean_p ** 2 + 0.5 + 0.4 * u[1].abs())])
    for ch, m in ((-3, 60.0), (-2, 600.0)):
        p[0, ch] = per * m * (1 + 0.01 * u[0, ch])
        p[0, ch] = p[0, ch].float().double()
        m_act = p[0, ch].sum() / count                        # the mean the table really holds
        p[1, ch] = per * (m_act ** 2 + 4.0) * (1 + 0.01 * (u[1, ch] - u[1, ch].mean()))
    p[0, -1] = per * 1.5
    p[1, -1] = per * 2.25 * (1 - 2.0 ** -20)
    return p.float()


def gated_fwd_inputs(shape, O):
    """(y NCHW, s, t, u, w, bias) of tests/test_gpu_se.py::test_gated_project_forward (also read by the CPU test of the gated
    operand's straddle share)"""
    N, H, W, Ci, Co = shape
    y = bf16r(O.det_uniform((N, Ci, H, W), 810))
    s, t = 1 + 0.3 * O.det_uniform((Ci,), 811), 0.2 * O.det_uniform((Ci,), 812)
    u = 2.0 * O.det_uniform((N, Ci), 813)
    w = bf16r(O.det_param("g.conv.weight", (Co, Ci, 1, 1), 3))
    bias = O.det_uniform((Co,), 814) * 0.1
    return y, s, t, u, w, bias
