"""CPU test of tests/intervals.py on its own: fp32 operands drawn inside random brackets (both signs, zeros, subnormals, brackets
that straddle zero, operands on a bracket's end), the operation evaluated in torch.float32, the result asserted inside the
corresponding interval operation by check_interval -- the way the bracket builders use them.  Then the checkers' edge cases."""
import pytest
import torch

from intervals import TINY32, Interval, check_interval, check_store_bound

N = 20000


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _points(g, emin, emax, zeros=True):
    """N fp32 values (as fp64): either sign, magnitudes 2^emin .. 2^emax (emin -149: subnormals), every 16th an exact zero"""
    e = torch.randint(emin, emax + 1, (N,), generator=g).double()
    m = 1 + torch.rand(N, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0).double()
    p = (sign * m * torch.pow(torch.tensor(2.0, dtype=torch.float64), e)).float().double()
    if zeros:
        p[::16] = 0.0
    return p


def _bracket(seed, emin=-149, emax=40, one_sign=False):
    """(Interval with fp32 ends, an fp32 operand inside it).  A third of the brackets have zero width, a third are narrow, a third
    join two independent points (half of those straddle zero); one_sign: a divisor's bracket, never containing zero.  Every 8th
    operand sits on the lower end, every 8th on the upper."""
    g = _gen(seed)
    p, q = _points(g, emin, emax, not one_sign), _points(g, emin, emax, not one_sign)
    if one_sign:
        q = q.abs() * torch.sign(p)
    kind = torch.arange(N) % 3
    narrow = (p * (1 + 2.0 ** -18 * torch.rand(N, generator=g, dtype=torch.float64))).float().double()
    q = torch.where(kind == 0, p, torch.where(kind == 1, narrow, q))
    lo, hi = torch.minimum(p, q), torch.maximum(p, q)
    t = torch.rand(N, generator=g, dtype=torch.float64)
    t[1::8], t[2::8] = 0.0, 1.0
    a = (lo + t * (hi - lo)).float().double().clamp(lo, hi)
    return Interval(lo, hi), a.float()


def _fmaf(a, b, c):
    """fmaf(a, b, c) of fp32 tensors, correctly rounded: the product is exact in fp64, the sum is rounded to odd there (TwoSum gives
    the sign of what the fp64 add lost), and fp64 -> fp32 of a round-to-odd value is the single rounding of the exact sum"""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(torch.int64)
    even = (bits & 1) == 0
    up = (err > 0) == (s > 0)                        # the exact sum is larger in magnitude than s
    bits = torch.where((err != 0) & even, torch.where(up, bits + 1, bits - 1), bits)
    return bits.view(torch.float64).float()


def test_operations_contain_the_fp32_result():
    A, a = _bracket(1)
    B, b = _bracket(2)
    Cc, c = _bracket(3)
    assert bool(((A.lo < 0) & (A.hi > 0)).any()) and bool((a == 0).any()) and bool(((a != 0) & (a.abs() < 2.0 ** -126)).any())
    assert bool((a.double() == A.lo).any()) and bool((a.double() == A.hi).any()) and bool((A.lo < A.hi).any())
    check_interval(a * b, A.mul(B, 1), "a*b", None)
    check_interval(a + b, A.add(B, 1), "a+b", None)
    check_interval(a - b, A.add(B, 1, -1.0), "a-b", None)
    check_interval(_fmaf(a, b, c), A.fma(B, Cc), "fmaf(a,b,c)", None)
    check_interval((a + b) - c, A.add(B, 1).add(Cc, 1, -1.0), "(a+b)-c", None)
    # mul carries no subnormal floor (check_interval's own 2^-149 covers a final product that is subnormal, not one that is
    # multiplied further): the chained product takes operands whose products stay normal
    (A, a), (B, b), (Cc, c) = _bracket(11, -30, 30), _bracket(12, -30, 30), _bracket(13, -30, 30)
    check_interval((a * b) * c, A.mul(B, 1).mul(Cc, 1), "(a*b)*c", None)
    check_interval(_fmaf(a, b, c) * c, A.fma(B, Cc).mul(Cc, 1), "fmaf(a,b,c)*c", None)
    # n = 0: exact, no rounding -- the fp64 product (exact for fp32 factors) and sum of fp32 operands lie inside as they are
    for exact, iv in ((a.double() * b.double(), A.mul(B, 0)), (a.double() + b.double(), A.add(B, 0)), (a.double() - b.double(), A.add(B, 0, -1.0))):
        assert bool(((exact >= iv.lo) & (exact <= iv.hi)).all())


def test_division_and_square_root_contain_the_fp32_result():
    A, a = _bracket(4, -100, 40)
    D, d = _bracket(5, -40, 40, one_sign=True)
    assert bool((D.lo > 0).any()) and bool((D.hi < 0).any()) and bool((D.lo < D.hi).any())
    check_interval(a / d, A.div(D, 1), "a/d", None)
    check_interval(a / d, A.div(D, 1, 2), "a/d at one ulp", None)
    S, s = _bracket(6)
    s = s.abs()                                      # the value is non-negative; its bracket may reach below zero
    S = Interval(torch.minimum(S.lo, s.double()), torch.maximum(S.hi, s.double()))
    assert bool((S.lo < 0).any())
    # (sqrtf as IEEE 754 and the GPU define it, correctly rounded: the fp64 root rounded to fp32, which double rounding cannot
    # spoil for a square root; the host library's own fp32 sqrt is not correctly rounded everywhere)
    check_interval(torch.sqrt(s.double()).float(), S.sqrt(), "sqrt(a)", None)
    assert bool((S.sqrt().lo >= 0).all())


def test_division_refuses_a_divisor_bracket_containing_zero():
    one = Interval.exact(1.0)
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0), (-1.0, 0.0), (0.0, 0.0)):
        with pytest.raises(AssertionError):
            one.div(Interval(torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64)))
    one.div(Interval(torch.tensor(2.0 ** -149, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64)))


def test_exact_takes_floats_and_tensors():
    like = torch.zeros(3, dtype=torch.float64)
    s = Interval.exact(0.1, like=like)
    assert s.lo.dtype == torch.float64 and s.lo.dim() == 0 and float(s.lo) == float(s.hi) == 0.1 and s.lo.device == like.device
    t = Interval.exact(torch.tensor([1.5, -2.0]))
    assert t.lo.dtype == torch.float64 and torch.equal(t.lo, t.hi) and torch.equal(t.D, t.lo.abs()) and torch.equal(t.val, t.lo)
    assert t.split_share() == 0.0 and torch.equal(t.mid, t.lo) and float(t.half.max()) == 0.0 and torch.equal(t.amax, t.lo.abs())


def test_check_interval_ends_nan_and_infinite_ends():
    lo = torch.tensor([1.0, -3.0, 0.0, 2.0 ** -140], dtype=torch.float64)
    hi = torch.tensor([1.5, -2.0, 0.0, 2.0 ** -139], dtype=torch.float64)
    iv = Interval(lo, hi)
    assert check_interval(lo.float(), iv, "on the lower end", None) <= 1.0
    assert check_interval(hi.float(), iv, "on the upper end", None) <= 1.0
    out = hi.float().clone()
    out[1] = -2.0 + 2.0 ** -22                       # one fp32 step above the upper end
    with pytest.raises(AssertionError, match="outside the per-element bound"):
        check_interval(out, iv, "past the end", None)
    out = lo.float().clone()
    out[2] = float("nan")
    with pytest.raises(AssertionError, match="outside the per-element bound"):
        check_interval(out, iv, "a NaN", None)
    inf = float("inf")
    iv = Interval(torch.tensor([inf, -inf, 1.0], dtype=torch.float64), torch.tensor([inf, -inf, 2.0], dtype=torch.float64))
    assert check_interval(torch.tensor([inf, -inf, 1.5]), iv, "infinite ends", None) <= 1.0
    for bad in ([3.4e38, -inf, 1.5], [inf, inf, 1.5], [inf, -inf, 2.5], [float("nan"), -inf, 1.5]):
        with pytest.raises(AssertionError, match="outside the per-element bound"):
            check_interval(torch.tensor(bad), iv, "infinite ends", None)
    allinf = Interval(torch.tensor([inf], dtype=torch.float64), torch.tensor([inf], dtype=torch.float64))
    assert check_interval(torch.tensor([inf]), allinf, "all infinite", None) == 0.0
    assert TINY32 == 2.0 ** -149


def test_check_store_bound_rejects_a_value_rounded_twice():
    """fp32 -> bf16 of a value pre-rounded to 10 significand bits: 1 + 2^-8 + 2^-11 lies above the middle of 1 and 1 + 2^-7 and
    rounds up; cut to 10 bits it IS the middle, and the tie goes to the even 1.0"""
    v = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -11], dtype=torch.float32)
    pre = torch.tensor([1 + 2.0 ** -8], dtype=torch.float32)
    once, twice = v.to(torch.bfloat16).float(), pre.to(torch.bfloat16).float()
    assert float(once) == 1 + 2.0 ** -7 and float(twice) == 1.0
    iv = Interval.exact(v)
    check_store_bound(once, iv, "rounded once", None)
    with pytest.raises(AssertionError, match=r"not in \[bf16\(lo\), bf16\(hi\)\]"):
        check_store_bound(twice, iv, "rounded twice", None)
    g = _gen(7)
    x = (torch.rand(4096, generator=g) + 1) * torch.pow(torch.tensor(2.0), torch.randint(-8, 9, (4096,), generator=g).float())
    pre10 = ((x.double() * 2.0 ** 9 / torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(x.double())))).round()
             * torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(x.double()))) / 2.0 ** 9).float()
    check_store_bound(x.to(torch.bfloat16).float(), Interval.exact(x), "random, rounded once", None)
    with pytest.raises(AssertionError, match=r"not in \[bf16\(lo\), bf16\(hi\)\]"):
        check_store_bound(pre10.to(torch.bfloat16).float(), Interval.exact(x), "random, rounded twice", None)
