"""CPU proof that the per-element bounds of tests/gpu_util.py bite.  A plain torch emulation of each kernel class's arithmetic
(fp32 operands formed from bf16 inputs, fp32 accumulate, round-to-nearest-even bf16 store) must sit inside its bound with every
condition of the helpers met; the same emulation with one fault -- a precision loss or a dropped / misplaced term of the kind an
optimisation of the kernels can introduce -- must be rejected.  Nothing here touches a kernel: the faults live in the emulation.
Shapes and input distributions are those of tests/test_gpu_kernels.py (5x5 depthwise 3x14x14x96, 1x1 600 pixels 96 -> 40)."""
import pytest
import torch

import gpu_util as G
from gpu_util import (Interval, act_interval, bf16r, check_dw_bound, check_onload_bound, check_red_bound, check_stats_bound,
                      check_sum_bound, dw_dgrad_terms, dw_elem_err, dw_fwd_terms, dw_wgrad_terms, dy_interval, off_hinge,
                      onload_dgrad_terms, onload_elem_err, onload_fwd_terms, pad_hw, wgrad_terms)


def _u(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _coefs(C_, seed):
    """bnbuf rows as gpu_util.rand_bn_coefs draws them"""
    u = _u((8, C_), seed)
    b = torch.zeros(8, C_)
    b[0], b[1], b[3], b[4], b[5], b[6] = 1 + 0.3 * u[0], 0.2 * u[1], 0.05 * u[3], 0.02 * u[4], 0.1 * u[5], 1 + 0.2 * u[6].abs()
    b[2] = b[0]
    return b


def _trunc_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _rejected(fn):
    with pytest.raises(AssertionError, match="outside the per-element bound"):
        fn()


# ---- emulations (fp32 throughout; every `fault` is one of the issue's list) -----------------------------------------------------
def emu_act(z, s, t, bf16, fault=None):
    if fault == "shift_dropped":
        t = t.clone()
        t[int(t.abs().argmax())] = 0.0
    a = torch.relu(z * s + t)                    # unfused fp32: product and sum rounded separately
    if fault == "trunc":
        return _trunc_bf16(a)
    return bf16r(a) if bf16 or fault == "operand_bf16" else a


def emu_dy(g, y, cf, bf16, fault=None):
    pre = y * cf[0] + cf[1]
    m = (pre >= 0) if fault == "mask_ge" else (pre > 0)
    d = cf[2] * (g * m) + (cf[3] * y + cf[4])
    return bf16r(d) if bf16 else d


def emu_gemm(a2, w2, bias=None, fault=None):
    """a2 (M,K) bf16 values, w2 (Co,K) bf16 values -> fp32 accumulator (M,Co)"""
    if fault == "acc_bf16_chunks":
        acc = torch.zeros(a2.shape[0], w2.shape[0])
        for k0 in range(0, a2.shape[1], 32):
            acc = bf16r(acc + a2[:, k0:k0 + 32] @ w2[:, k0:k0 + 32].t())
    else:
        acc = a2 @ w2.t()
    if bias is not None:
        b = bias.clone()
        if fault == "bias_missing":
            b[int(b.abs().argmax())] = 0.0
        acc = acc + b
    return acc


def emu_dw_fwd(a, w, bias, fault=None, corner=None):
    """a (N,H,W,C) fp32 operand, w (C,k,k) -> fp32 accumulator"""
    N, H, W, C_ = a.shape
    k = w.shape[-1]
    p = k // 2
    if fault == "weights_bf16":
        w = bf16r(w)
    ap = pad_hw(a, p)
    if fault == "corner":                         # the padded corner above-left of pixel (0, 0) read as relu(shift)
        ap[:, p - 1, p - 1] = corner
    acc = bias.expand(N, H, W, C_).clone() if bias is not None else torch.zeros_like(a)
    for kh in range(k):
        for kw in range(k):
            term = ap[:, kh:kh + H, kw:kw + W] * w[:, kh, kw]
            if fault == "tap_last_row" and kh == 0 and kw == 0:
                term = term.clone()
                term[:, H - 1] = 0.0
            acc = acc + term
    return acc


def emu_dw_dgrad(d, w, fault=None):
    N, H, W, C_ = d.shape
    k = w.shape[-1]
    p = k // 2
    if fault == "weights_bf16":
        w = bf16r(w)
    gp = torch.zeros(N, H + 2 * p, W + 2 * p, C_)
    for kh in range(k):
        for kw in range(k):
            gp[:, kh:kh + H, kw:kw + W] += d * w[:, kh, kw]
    return gp[:, p:p + H, p:p + W]


# ---- MFMA launches with an on-load operand ------------------------------------------------------------------------------------
class _Pw:
    M, Ci, Co = 600, 96, 40

    def __init__(self):
        self.z = bf16r(_u((1, 1, self.M, self.Ci), 1))
        self.w = bf16r(_u((self.Co, self.Ci, 1, 1), 2) * (3.0 / self.Ci) ** 0.5)
        self.bias = 0.1 * _u((self.Co,), 3)
        self.sc, self.sh = 1 + 0.3 * _u((self.Ci,), 4), 0.2 * _u((self.Ci,), 5)
        self.iv = act_interval(self.z, self.sc, self.sh, bf16=True)
        self.terms = onload_fwd_terms(self.iv, self.w, self.bias)

    def acc(self, fault=None):
        a = emu_act(self.z, self.sc, self.sh, True, fault)
        return emu_gemm(a.view(self.M, self.Ci), self.w.view(self.Co, self.Ci), self.bias, fault).view(1, 1, self.M, self.Co)

    def check(self, fault=None):
        ref, slack, S = self.terms
        return check_onload_bound(bf16r(self.acc(fault)), ref, slack, S, self.Ci, "1x1 forward %s" % fault, family=None)


@pytest.fixture(scope="module")
def pw():
    return _Pw()


def test_mfma_forward_emulation_inside_bound(pw):
    worst = pw.check()
    assert 0.3 < worst <= 1.0, worst
    assert pw.iv.split_share() <= G.MAX_ACT_SPLIT


@pytest.mark.parametrize("fault", ["trunc", "acc_bf16_chunks", "shift_dropped", "bias_missing"])
def test_mfma_forward_faults_rejected(pw, fault):
    _rejected(lambda: pw.check(fault))


class _PwD:
    """1x1 input gradient, dy-on-load; channel 0 has shift 0 and y holds exact zeros there (the exact-zero side of the hinge)"""
    M, Ci, Co = 600, 40, 96

    def __init__(self):
        self.cf = _coefs(self.Co, 9)
        self.cf[1, 0] = 0.0
        self.g = bf16r(_u((1, 1, self.M, self.Co), 6))
        y = bf16r(_u((1, 1, self.M, self.Co), 7))
        y[..., ::7, 0] = 0.0
        self.y = off_hinge(y, self.cf[0], self.cf[1])
        assert int((self.y[..., 0] == 0).sum()) >= 80
        self.w = bf16r(_u((self.Co, self.Ci, 1, 1), 2) * (3.0 / self.Co) ** 0.5)
        self.resid = bf16r(_u((1, 1, self.M, self.Ci), 5))
        self.iv = dy_interval(self.g, self.y, self.cf, bf16=True)
        self.terms = onload_dgrad_terms(self.iv, self.w, 1, self.M, resid=self.resid)

    def check(self, fault=None):
        d = emu_dy(self.g, self.y, self.cf, True, fault)
        acc = d.view(self.M, self.Co) @ self.w.view(self.Co, self.Ci) + self.resid.view(self.M, self.Ci)
        ref, slack, S = self.terms
        return check_onload_bound(bf16r(acc).view(1, 1, self.M, self.Ci), ref, slack, S, self.Co, "1x1 dgrad %s" % fault, family=None)


@pytest.fixture(scope="module")
def pwd():
    return _PwD()


def test_mfma_dgrad_emulation_inside_bound(pwd):
    worst = pwd.check()
    assert 0.3 < worst <= 1.0, worst
    assert pwd.iv.split_share() <= G.MAX_DY_SPLIT


def test_mask_taken_with_ge_on_exact_zeros_rejected(pwd):
    _rejected(lambda: pwd.check("mask_ge"))


def test_hinge_conditions_are_asserted():
    s, t = torch.ones(8), torch.zeros(8)
    v = bf16r(_u((50, 8), 1)) * 1e-3                     # everything on the hinge
    with pytest.raises(AssertionError, match="off_hinge would move"):
        off_hinge(v, s, t)
    with pytest.raises(AssertionError, match="on the ReLU hinge"):
        G.relu_mask(v, s, t)
    with pytest.raises(AssertionError, match="straddle a rounding boundary"):
        # shifts of 2^20 make the interval wider than a bf16 ulp of most elements
        act_interval(bf16r(_u((50, 8), 2)), torch.full((8,), 2.0 ** 10), torch.full((8,), 3.0 * 2.0 ** 17), bf16=True)


# ---- depthwise sweeps -----------------------------------------------------------------------------------------------------------
class _Dw:
    N, H, W, C = 3, 14, 14, 96

    def __init__(self, k):
        self.k = k
        self.z = bf16r(_u((self.N, self.H, self.W, self.C), 1))
        self.w = _u((self.C, k, k), 2) * (1.0 / k)                  # fp32, NOT rounded to bf16
        self.bias = 0.1 * _u((self.C,), 3)
        self.sc, self.sh = 1 + 0.3 * _u((self.C,), 4), 0.2 * _u((self.C,), 5)
        self.a = act_interval(self.z, self.sc, self.sh, bf16=False)
        self.fwd = dw_fwd_terms(self.a, self.w, self.bias)
        self.cf = _coefs(self.C, 9)
        self.g = bf16r(_u((self.N, self.H, self.W, self.C), 6))
        self.y = off_hinge(bf16r(_u((self.N, self.H, self.W, self.C), 7)), self.cf[0], self.cf[1])
        self.d = dy_interval(self.g, self.y, self.cf, bf16=False)
        self.dg = dw_dgrad_terms(self.d, self.w, self.H, self.W)

    def check_fwd(self, fault=None):
        a = emu_act(self.z, self.sc, self.sh, False, fault)
        acc = emu_dw_fwd(a, self.w, self.bias, fault, corner=torch.relu(self.sh))
        return check_dw_bound(bf16r(acc), self.fwd[0], self.fwd[1], self.k, "dw%d forward %s" % (self.k, fault), family=None)

    def check_dgrad(self, fault=None):
        d = emu_dy(self.g, self.y, self.cf, fault == "operand_bf16")
        return check_dw_bound(bf16r(emu_dw_dgrad(d, self.w, fault)), self.dg[0], self.dg[1], self.k, "dw%d dgrad %s" % (self.k, fault), family=None)


@pytest.fixture(scope="module", params=[3, 5])
def dw(request):
    return _Dw(request.param)


def test_depthwise_emulations_inside_bound(dw):
    assert 0.3 < dw.check_fwd() <= 1.0
    assert 0.3 < dw.check_dgrad() <= 1.0


@pytest.mark.parametrize("fault", ["weights_bf16", "operand_bf16", "shift_dropped", "corner", "tap_last_row"])
def test_depthwise_forward_faults_rejected(dw, fault):
    _rejected(lambda: dw.check_fwd(fault))


@pytest.mark.parametrize("fault", ["weights_bf16", "operand_bf16"])
def test_depthwise_dgrad_faults_rejected(dw, fault):
    _rejected(lambda: dw.check_dgrad(fault))


def test_depthwise_wgrad_emulation_inside_bound(dw):
    a = emu_act(dw.z, dw.sc, dw.sh, False)
    d = emu_dy(dw.g, dw.y, dw.cf, False)
    k, p = dw.k, dw.k // 2
    ap = pad_hw(a, p)
    got = torch.stack([torch.stack([(ap[:, kh:kh + dw.H, kw:kw + dw.W] * d).sum((0, 1, 2)) for kw in range(k)], -1) for kh in range(k)], -2)
    ref, S, slack = dw_wgrad_terms(dw.a, dw.d, k)
    M = dw.N * dw.H * dw.W
    assert check_sum_bound(got, ref, S, M, 1, 2, "dw%d wgrad" % k, slack, family=None) <= 1.0
    _rejected(lambda: check_sum_bound(got * (1 + 2.0 ** -9), ref, S, M, 1, 2, "dw%d wgrad scaled by 1 + 2^-9" % k, slack, family=None))


# ---- fp32 sums: weight gradient, statistics, reduce -----------------------------------------------------------------------------
def test_wgrad_emulation_inside_bound(pw, pwd):
    """1x1 weight gradient over act-on-load x (96 channels) and dy-on-load (96 channels of _PwD), both staged as bf16"""
    a = emu_act(pw.z, pw.sc, pw.sh, True).view(pw.M, pw.Ci)
    d = emu_dy(pwd.g, pwd.y, pwd.cf, True).view(pwd.M, pwd.Co)
    P = 3
    parts = [d[i::P].t() @ a[i::P] for i in range(P)]
    got = (parts[0] + parts[1]) + parts[2]
    ref, S, slack = wgrad_terms(pw.iv, pwd.iv, 1)
    worst = check_sum_bound(got.view(ref.shape), ref, S, pw.M, P, 1, "1x1 wgrad", slack, family=None)
    assert worst <= 1.0
    # an operand truncated instead of rounded moves the sum out of its bound
    at = _trunc_bf16(torch.relu(pw.z * pw.sc + pw.sh)).view(pw.M, pw.Ci)
    _rejected(lambda: check_sum_bound((d.t() @ at).view(ref.shape), ref, S, pw.M, P, 1, "1x1 wgrad trunc", slack, family=None))


def _sparse_pixels(M, tile, seg):
    """first and last pixel, both sides of the first tile boundary and of a workgroup boundary"""
    return sorted({0, tile - 1, tile, seg - 1, seg, M - 1})


def test_sparse_probe_sees_a_dropped_pixel_in_wgrad():
    M, Ci, Co = 600, 96, 40
    px = _sparse_pixels(M, 64, 320)
    x, dy = torch.zeros(1, 1, M, Ci), torch.zeros(1, 1, M, Co)
    x[0, 0, px], dy[0, 0, px] = bf16r(_u((len(px), Ci), 1)), bf16r(_u((len(px), Co), 2))
    ref, S, slack = wgrad_terms(Interval.exact(x), Interval.exact(dy), 1)
    assert float(slack.abs().max()) == 0.0
    got = dy.view(M, Co).t() @ x.view(M, Ci)
    assert check_sum_bound(got.view(ref.shape), ref, S, M, 3, 1, "sparse wgrad", slack, family=None) <= 1.0
    for drop in (M - 1, 0, 64):
        keep = torch.ones(M, 1)
        keep[drop] = 0
        bad = (dy.view(M, Co) * keep).t() @ x.view(M, Ci)
        _rejected(lambda: check_sum_bound(bad.view(ref.shape), ref, S, M, 3, 1, "sparse wgrad, pixel %d dropped" % drop, slack, family=None))
    dbl = got + dy.view(M, Co)[M - 1:].t() @ x.view(M, Ci)[M - 1:]
    _rejected(lambda: check_sum_bound(dbl.view(ref.shape), ref, S, M, 3, 1, "sparse wgrad, last pixel doubled", slack, family=None))


def test_statistics_and_sparse_probe(pw):
    ref, slack, S = pw.terms
    e = onload_elem_err(slack, S, pw.Ci)
    v = pw.acc()
    P = 13
    st = torch.stack([torch.stack([v.view(pw.M, pw.Co)[i::P].sum(0) for i in range(P)], -1),
                      torch.stack([(v * v).view(pw.M, pw.Co)[i::P].sum(0) for i in range(P)], -1)])
    assert check_stats_bound(st, ref, e, pw.M, "1x1 forward", family=None) <= 1.0
    # sparse probe: plain x, no bias, six live pixels
    px = _sparse_pixels(pw.M, 64, 320)
    x = torch.zeros(1, 1, pw.M, pw.Ci)
    x[0, 0, px] = bf16r(_u((len(px), pw.Ci), 11))
    r, k, S = onload_fwd_terms(Interval.exact(x), pw.w)
    e = onload_elem_err(k, S, pw.Ci)
    v = emu_gemm(x.view(pw.M, pw.Ci), pw.w.view(pw.Co, pw.Ci))
    tab = lambda v: torch.stack([v.sum(0), (v * v).sum(0)]).unsqueeze(-1)
    assert check_stats_bound(tab(v), r, e, pw.M, "sparse statistics", family=None) <= 1.0
    v2 = v.clone()
    v2[pw.M - 1] = 0
    _rejected(lambda: check_stats_bound(tab(v2), r, e, pw.M, "sparse statistics, last pixel dropped", family=None))


def test_reduce_emulation_and_sparse_probe():
    M, C_ = 600, 40
    bn = _coefs(C_, 22)
    y = off_hinge(bf16r(_u((M, C_), 21)), bn[0], bn[1])
    gq = bf16r(_u((M, C_), 23))

    def red(gq, drop=None):
        dz = gq * ((y * bn[0] + bn[1]) > 0)
        if drop is not None:
            dz = dz.clone()
            dz[drop] = 0
        xhat = y * bn[6] + (-bn[5] * bn[6])
        return torch.stack([dz.sum(0), (dz * xhat).sum(0)]).unsqueeze(-1)
    assert check_red_bound(red(gq), gq, y, bn, M, "reduce", family=None) <= 1.0
    sp = torch.zeros(M, C_)
    px = _sparse_pixels(M, 64, 320)
    sp[px] = gq[px]
    assert check_red_bound(red(sp), sp, y, bn, M, "sparse reduce", family=None) <= 1.0
    _rejected(lambda: check_red_bound(red(sp, drop=M - 1), sp, y, bn, M, "sparse reduce, last pixel dropped", family=None))


def test_dw_statistics_emulation(dw):
    ref, S = dw.fwd
    v = emu_dw_fwd(emu_act(dw.z, dw.sc, dw.sh, False), dw.w, dw.bias)
    st = torch.stack([v.sum((0, 1, 2)), (v * v).sum((0, 1, 2))]).unsqueeze(-1)
    M = dw.N * dw.H * dw.W
    assert check_stats_bound(st, ref, dw_elem_err(S, dw.k), M, "dw%d forward" % dw.k, family=None) <= 1.0
