"""Interval arithmetic for the per-element error bounds of the GPU tests; it knows no kernel.
u = 2^-24 is the unit roundoff of fp32 (round to nearest).  The host never re-enacts the device's fp32 evaluation: it brackets it in
fp64 by an interval [lo, hi] that every correctly rounded evaluation (fused or not) falls into.  Rounding (to fp32 or to bf16) is
monotone, so a stored value lies between the rounded ends of its bracket.  Nothing here is fitted to a kernel's output.  Two shapes
of check: an Interval that already holds EVERY rounding up to the stored fp32 value (check_interval), and an Interval of the fp32
value that is then rounded once to bf16 (check_store_bound); sums get check_sum_bound's form.  The kernel-specific brackets are in
bounds_conv.py, bounds_se.py, bounds_tail.py and bounds_mlabel.py."""
import torch

U32 = 2.0 ** -24
TINY32 = 2.0 ** -149     # one fp32 denormal step: the absolute floor of a rounding whose result is subnormal
D64 = 2.0 ** -48         # relative allowance for a chain of at most 32 double-precision operations (each 2^-53)
E64 = 2.0 ** -52         # one double ulp, relative

WORST = {}          # family -> largest measured error / bound (printed by the tests; DESIGN.md section 6 records them)
SHARES = {}         # largest measured shares: split bf16 elements per operand kind (to_bf16), elements on the ReLU hinge


def round32(x):
    """round a double tensor to fp32 (to nearest even) and back: monotone, so it maps a bracket's ends to the rounded bracket's"""
    return x.float().double()


def round_bf16(t):
    """fp64 -> fp32 -> bf16 (both round to nearest even) -> fp64: monotone, so it maps an interval's ends to the ends of the
    interval of rounded values"""
    return t.float().to(torch.bfloat16).double()


def f32(v):
    """a Python float holding the fp32 value the C ABI passes for v"""
    return float(torch.tensor(v, dtype=torch.float32))


def widen(lo, hi, n=1, ulps=1, floor=False, host=0.0):
    """n further fp32 roundings (of ulps * u each: 2 for a one-ulp function) of a value known to lie in [lo, hi]: each moves it by at
    most ulps * u of its own magnitude, so the result lies in [lo - f|lo|, hi + f|hi|] with f = (1 + ulps u)^n - 1 (a value of the
    other sign than an end is inside anyway).  host: the relative error of the host's own fp64 evaluation of lo and hi (D64), added
    to f.  floor: the absolute floor 2^-149 of each rounding whose result is subnormal."""
    f = (1 + ulps * U32) ** n - 1 + host
    lo, hi = lo - f * lo.abs(), hi + f * hi.abs()
    return (lo - n * TINY32, hi + n * TINY32) if floor else (lo, hi)


def widen64(lo, hi, n=1):
    """n double roundings (or n one-ulp double functions) of a value in [lo, hi]"""
    return lo - n * E64 * lo.abs(), hi + n * E64 * hi.abs()


def store32(lo, hi, mag=None):
    """a double result in [lo, hi] (computed with double error D64 of `mag`, default its own magnitude) stored as fp32"""
    m = torch.maximum(lo.abs(), hi.abs()) if mag is None else mag
    return Interval(*widen(lo - D64 * m, hi + D64 * m, 1))


def hull(*ts):
    """(min, max) over tensors broadcast against each other: the range of a function that is monotone in each argument, from its
    values at the corners"""
    c = torch.stack(torch.broadcast_tensors(*ts))
    return c.min(0).values, c.max(0).values


class Interval:
    """an operand tensor known to lie in [lo, hi] element by element (fp64)"""

    def __init__(self, lo, hi, D=None, val=None):
        """D: the magnitude the operand's rounding is relative to; val: the exact (fp64) value of the operand"""
        assert bool((lo <= hi).all())
        self.lo, self.hi, self.D, self.val = lo, hi, D, val

    @staticmethod
    def exact(x, device=None, like=None):
        """x known exactly: a tensor, or a float scalar (0-dim), moved to `device` / `like`'s device where one is given"""
        device = device if like is None else like.device
        if not torch.is_tensor(x):
            x = torch.tensor(x, dtype=torch.float64, device=device)
        x = x.double() if device is None else x.to(device=device, dtype=torch.float64)
        return Interval(x, x, x.abs(), x)

    @property
    def mid(self):
        return (self.lo + self.hi) / 2

    @property
    def half(self):
        return (self.hi - self.lo) / 2

    @property
    def amax(self):
        return torch.maximum(self.lo.abs(), self.hi.abs())

    def split_share(self):
        return float((self.lo != self.hi).double().mean())

    # ---- fl(op) of operands anywhere inside their brackets; n fp32 roundings, n = 0: exact, no rounding ----
    def mul(self, b, n=1):
        """Interval of fl(a*b) for a in [a.lo, a.hi], b in [b.lo, b.hi]: hull of the four corner products (a product is monotone in
        each factor), widened by n roundings"""
        lo, hi = hull(self.lo * b.lo, self.lo * b.hi, self.hi * b.lo, self.hi * b.hi)
        return Interval(*widen(lo, hi, n)) if n else Interval(lo, hi)

    def add(self, b, n=1, sign=1.0):
        """Interval of fl(a + sign*b): the exact sum of the ends, widened by n roundings"""
        lo, hi = (self.lo + b.lo, self.hi + b.hi) if sign > 0 else (self.lo - b.hi, self.hi - b.lo)
        return Interval(*widen(lo, hi, n, floor=True)) if n else Interval(lo, hi)

    def div(self, b, n=1, ulps=1):
        """Interval of fl(a / b), b of one sign and never zero: hull of the corner quotients, n roundings of ulps * u each"""
        assert bool(((b.lo > 0) | (b.hi < 0)).all())
        lo, hi = hull(self.lo / b.lo, self.lo / b.hi, self.hi / b.lo, self.hi / b.hi)
        return Interval(*widen(lo, hi, n, ulps, True, D64))

    def sqrt(self):
        """Interval of sqrtf(a) (IEEE: correctly rounded, monotone); a negative lower end of a bracket of a non-negative value is 0"""
        lo, hi = widen(torch.sqrt(self.lo.clamp_min(0.0)) * (1 - D64), torch.sqrt(self.hi.clamp_min(0.0)) * (1 + D64), 1, floor=True)
        return Interval(lo.clamp_min(0.0), hi)

    def fma(self, a, c):
        """Interval of fmaf(s, a, c): the exact product plus c, rounded once"""
        return self.mul(a, 0).add(c, 1)


def to_bf16(iv, cap, what):
    """iv rounded to bf16 (pack8 / pack_bf16: round to nearest even) at both ends, D and val kept.  Asserted: at most `cap` of the
    elements have lo != hi (the interval straddles a rounding boundary); the largest share met is kept in SHARES[what]."""
    out = Interval(round_bf16(iv.lo), round_bf16(iv.hi), iv.D, iv.val)
    share = out.split_share()
    assert share <= cap, "%s operand: %.3g of the bf16 elements straddle a rounding boundary (limit %.3g)" % (what, share, cap)
    SHARES[what] = max(SHARES.get(what, 0.0), share)
    return out


def _assert_bound(hip, ref, bound, what, family):
    hip, ref, bound = hip.double(), ref.double(), bound.double()
    assert hip.shape == ref.shape == bound.shape, (what, hip.shape, ref.shape, bound.shape)
    err = (hip - ref).abs()
    bad = ~(err <= bound)                     # (a NaN fails)
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        idx = tuple(int(v) for v in torch.unravel_index(ratio.reshape(-1).argmax(), ratio.shape)) if ratio.dim() else ()
        raise AssertionError("%s: %d of %d elements outside the per-element bound; worst at %s: got %r, fp64 %r, |err| %.3e > bound %.3e (x%.2f)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(hip[idx]), float(ref[idx]), float(err[idx]),
                                float(bound[idx]), float(err[idx] / bound[idx].clamp_min(1e-300))))
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    if family:
        WORST[family] = max(WORST.get(family, 0.0), worst)
    return worst


def check_interval(hip, iv, what, family):
    """hip: an fp32 output whose EVERY rounding is already inside iv: lo - 2^-149 <= hip <= hi + 2^-149 for every element (asserted
    on the ends themselves: an output may sit exactly on one).  Returns max |hip - mid| / (half + 2^-149), also kept in WORST.
    A bracket with an infinite end: where lo == hi == +-inf the output must equal it; those elements stay out of the ratio."""
    h = hip.double()
    lo, hi = iv.lo.to(h.device), iv.hi.to(h.device)
    assert h.shape == lo.shape, (what, h.shape, lo.shape)
    inf = torch.isinf(lo) & (lo == hi)
    if bool(inf.any()):
        assert bool((h[inf] == lo[inf]).all()), "%s: outside the per-element bound (an infinite result expected)" % what
        if bool(inf.all()):
            return 0.0
        h, lo, hi = h[~inf], lo[~inf], hi[~inf]
    bad = ~((h >= lo - TINY32) & (h <= hi + TINY32))          # (a NaN fails)
    ratio = (h - (lo + hi) / 2).abs() / ((hi - lo) / 2 + TINY32)
    if bool(bad.any()):
        r = torch.where(bad, ratio, torch.zeros_like(ratio))
        idx = tuple(int(v) for v in torch.unravel_index(r.reshape(-1).argmax(), r.shape)) if r.dim() else ()
        raise AssertionError("%s: %d of %d elements outside the per-element bound; worst at %s: got %r, bracket [%r, %r] (x%.2f)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(h[idx]), float(lo[idx]), float(hi[idx]), float(ratio[idx])))
    worst = min(1.0, float(ratio.max())) if ratio.numel() else 0.0       # (an element exactly on an end: 1 up to the fp64 rounding of mid)
    if family:
        WORST[family] = max(WORST.get(family, 0.0), worst)
    return worst


def check_store_bound(hip, iv, what, family):
    """A bf16 elementwise store (pack8: round to nearest even) of an fp32 value known to lie in iv = [lo, hi]: rounding is monotone,
    so EVERY element lies in [bf16(lo), bf16(hi)] -- asserted as such (it is what rejects a value rounded twice) -- and therefore
    within 2^-8 (|mid| + half) + half of mid, which is what the ratio in WORST is taken against."""
    h = hip.double()
    lo, hi = round_bf16(iv.lo).to(h.device), round_bf16(iv.hi).to(h.device)
    assert h.shape == lo.shape, (what, h.shape, lo.shape)
    bad = ~((h >= lo) & (h <= hi))
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside the per-element bound (not in [bf16(lo), bf16(hi)]); first at %s: got %r, bracket [%r, %r]"
                             % (what, int(bad.sum()), bad.numel(), idx, float(h[idx]), float(lo[idx]), float(hi[idx])))
    mid, half = iv.mid.to(h.device), iv.half.to(h.device)
    return _assert_bound(h, mid, 2.0 ** -8 * (mid.abs() + half) + half, what, family)


def sum_bound(S, M, P, c, slack=None):
    """check_sum_bound's bound as a tensor: (c*M + P + 1)*2^-22*S + slack"""
    b = (c * M + P + 1) * 2.0 ** -22 * S.double()
    return b if slack is None else b + slack.double()


def sum_interval(ref, S, M, P, c, slack=None):
    """the fp32 sum of check_sum_bound as an Interval, for a result that is processed further (times a factor, through a relu)"""
    b = sum_bound(S, M, P, c, slack)
    return Interval(ref.double() - b, ref.double() + b)


def check_sum_bound(hip, ref, S, M, P, c, what, slack=None, family="fp32 sums"):
    """Bound for an fp32 sum of M terms per output, written as P partial slabs / columns that a finalize (or the host) adds:
    weight-gradient partials after mnas_wgrad_finalize, BatchNorm statistics (sum y, sum y^2), the fused reduce (sum dz,
    sum dz*xhat).  ref: the fp64 sum; S: the same sum over absolute values.  Every add loses at most 2^-24 of a running
    magnitude <= S (M in the kernel, P in the finalize, 1 for an accumulate target or bias); a term that is itself rounded (c = 2:
    fp32 x fp32 products of the depthwise weight gradient, xhat = fma(y, inv, m), y^2) doubles the per-term loss, an exact term
    (c = 1: bf16 x bf16) does not; the whole is doubled as in check_gemm_bound:
        |hip - ref| <= (c*M + P + 1)*2^-22*S + slack.
    slack: what the exact sum over any operands inside their intervals may differ from ref by -- for two interval operands a, b
    sum(|a.mid|*b.half + |b.mid|*a.half + a.half*b.half) (prod_slack); for statistics of an fp32 accumulator, the sum of the
    elements' own fp32 error (onload_elem_err / dw_elem_err)."""
    return _assert_bound(hip, ref, sum_bound(S, M, P, c, slack), what, family)
