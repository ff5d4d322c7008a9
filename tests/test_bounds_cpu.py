"""CPU proof that the per-element bounds of tests/bounds_*.py bite.  A plain torch emulation of each kernel class's arithmetic
(fp32 operands formed from bf16 inputs, fp32 accumulate, round-to-nearest-even bf16 store) must sit inside its bound with every
condition of the helpers met; the same emulation with one fault -- a precision loss or a dropped / misplaced term of the kind an
optimisation of the kernels can introduce -- must be rejected.  Nothing here touches a kernel: the faults live in the emulation.
Shapes and input distributions are those of tests/test_gpu_kernels.py (5x5 depthwise 3x14x14x96, 1x1 600 pixels 96 -> 40)."""
import numpy as np
import pytest
import torch

import bounds_conv as BC
import bounds_mlabel as BM
import bounds_se as BS
import bounds_tail as BT
import intervals as IV
from bounds_conv import (act_interval, check_dw_bound, check_onload_bound, check_red_bound, check_stats_bound, dw_dgrad_terms, dw_elem_err,
                         dw_fwd_terms, dw_wgrad_terms, dy_interval, off_hinge, onload_dgrad_terms, onload_elem_err, onload_fwd_terms,
                         wgrad_terms)
from gpu_util import bf16r
from intervals import Interval, check_sum_bound
from refs64 import pad_hw


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
    assert pw.iv.split_share() <= BC.MAX_ACT_SPLIT


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
    assert pwd.iv.split_share() <= BC.MAX_DY_SPLIT


def test_mask_taken_with_ge_on_exact_zeros_rejected(pwd):
    _rejected(lambda: pwd.check("mask_ge"))


def test_hinge_conditions_are_asserted():
    s, t = torch.ones(8), torch.zeros(8)
    v = bf16r(_u((50, 8), 1)) * 1e-3                     # everything on the hinge
    with pytest.raises(AssertionError, match="off_hinge would move"):
        off_hinge(v, s, t)
    with pytest.raises(AssertionError, match="on the ReLU hinge"):
        BC.relu_mask(v, s, t)
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


# ---- squeeze-excite, stem gradients, glue, finalizes ----------------------------------------------------------------------------
# The device's sigmoid is modelled as the fp64 value moved 0.8 of the way to an end of its bracket (end = -1, 0, +1) and rounded to
# fp32; everything else is fp32 torch arithmetic in the kernels' operation order where the kernels fix one.
def _sig(v, end=0):
    iv = BS.sigmoid_interval(v)
    return (iv.val + 0.8 * end * (iv.hi - iv.val if end > 0 else iv.val - iv.lo)).float()


def _ok(r):
    print("ratio %.3f" % r)
    assert r <= 1.0
    return r


def test_sigmoid_bracket_and_faults():
    v = torch.cat([torch.arange(-30 * 64, 30 * 64 + 1).float() / 64, torch.tensor([0.0, -0.0])])
    iv = BS.sigmoid_interval(v)
    got = 1.0 / (1.0 + torch.exp(-v))                      # fp32, a correctly rounded exponential
    assert 0.05 < _ok(IV.check_interval(got, iv, "sigmoid", None))
    for end in (-1, 1):
        _ok(IV.check_interval(_sig(v, end), iv, "sigmoid end %d" % end, None))
    _rejected(lambda: IV.check_interval(bf16r(got), iv, "sigmoid rounded to bf16", None))
    # du = acc * sg * (1 - sg)
    acc = _u(v.shape, 1)
    du_iv = Interval.exact(acc).mul(BS.sig1m_interval(v), 1)
    for end in (-1, 0, 1):
        sg = _sig(v, end)
        _ok(IV.check_interval(acc * sg * (1.0 - sg), du_iv, "du end %d" % end, None))
    _rejected(lambda: IV.check_interval(acc * _sig(v), du_iv, "du without 1 - sg", None))
    sgb = bf16r(_sig(v))
    _rejected(lambda: IV.check_interval(acc * sgb * (1.0 - sgb), du_iv, "du with a bf16 sigmoid", None))


class _Se:
    N, H, W, C = 2, 14, 14, 48

    def __init__(self, amp=2.0):
        sh = (self.N, self.H, self.W, self.C)
        self.HW = self.H * self.W
        self.z = bf16r(_u(sh, 31))
        self.s, self.t = 1 + 0.3 * _u((self.C,), 32), 0.2 * _u((self.C,), 33)
        self.u = amp * _u((self.N, self.C), 34)
        self.gs = bf16r(_u(sh, 35))
        self.dz = _u((self.N, self.C), 36)
        self.gate = BS.sigmoid_interval(self.u)
        self.g4 = BS.gate_nhwc(self.gate, sh)

    def sg(self, end=0):
        return _sig(self.u, end).view(self.N, 1, 1, self.C)


@pytest.fixture(scope="module", params=[2.0, 12.0])
def se(request):
    return _Se(request.param)


@pytest.mark.parametrize("virt", [True, False])
def test_se_scale_emulation_and_faults(se, virt):
    iv = BS.gated_act_interval(se.z, se.s if virt else None, se.t if virt else None, se.g4, bf16=False)
    a = emu_act(se.z, se.s, se.t, False) if virt else se.z
    for end in (-1, 0, 1):
        _ok(IV.check_store_bound(bf16r(a * se.sg(end)), iv, "se_scale end %d" % end, None))
    if virt:            # (a plain input is a bf16 value already: there is no rounding to do twice)
        _rejected(lambda: IV.check_store_bound(bf16r(bf16r(a) * se.sg()), iv, "se_scale: value rounded before the gate", None))
        _rejected(lambda: IV.check_store_bound(bf16r(emu_act(se.z, se.s, se.t, False, "shift_dropped") * se.sg()), iv, "se_scale: shift dropped", None))


def test_gated_mfma_operand_emulation_and_faults(se):
    Co = 16
    w = bf16r(_u((Co, se.C, 1, 1), 37) * (3.0 / se.C) ** 0.5)
    bias = 0.1 * _u((Co,), 38)
    iv = BS.gated_act_interval(se.z, se.s, se.t, se.g4, bf16=True)
    assert iv.split_share() <= BC.MAX_ACT_SPLIT
    ref, slack, S = onload_fwd_terms(iv, w, bias)
    M = se.N * se.HW

    def run(a):
        acc = emu_gemm(a.reshape(M, se.C), w.view(Co, se.C), bias).view(se.N, se.H, se.W, Co)
        return check_onload_bound(bf16r(acc), ref, slack, S, se.C, "gated 1x1 forward", family=None)
    a = emu_act(se.z, se.s, se.t, False)
    _ok(run(bf16r(a * se.sg())))
    _rejected(lambda: run(bf16r(bf16r(a) * se.sg())))                       # two roundings
    _rejected(lambda: run(bf16r(emu_act(se.z, se.s, se.t, False, "shift_dropped") * se.sg())))


def _emu_se_reduce(se, a, fault=None):
    """k_se_bwd_reduce + k_se_bwd_finish: per split, lane pr walks pixels p0+pr, p0+pr+R, ... with one fma each; lanes, then splits,
    added in order"""
    G_, R, chunk, splits = BS.se_geom(se.N, se.HW, se.C)
    assert (R, chunk, splits) == (42, 126, 2)
    g, a = se.gs.reshape(se.N, se.HW, se.C), a.reshape(se.N, se.HW, se.C)
    parts = []
    for sp in range(splits):
        p0, p1 = sp * chunk, min(se.HW, (sp + 1) * chunk)
        lanes = torch.zeros(R, se.N, se.C)
        for pr in range(R):
            acc = torch.zeros(se.N, se.C)
            for p in range(p0 + pr, p1, R):
                if fault == "drop_chunk_last" and p == chunk - 1:
                    continue
                acc = acc + g[:, p] * a[:, p]
                if fault == "acc_bf16":
                    acc = bf16r(acc)
                if fault == "double_split_first" and p == chunk:
                    acc = acc + g[:, p] * a[:, p]
            lanes[pr] = acc
        v = torch.zeros(se.N, se.C)
        for pr in range(R):
            v = v + lanes[pr]
        parts.append(v)
    v = torch.zeros(se.N, se.C)
    for p_ in parts:
        v = v + p_
    sg = _sig(se.u)
    return v * sg * (1.0 - sg)


@pytest.mark.parametrize("virt", [True, False])
def test_se_bwd_reduce_emulation_and_faults(se, virt):
    G_, R, chunk, splits = BS.se_geom(se.N, se.HW, se.C)
    aiv = act_interval(se.z, se.s, se.t, bf16=False) if virt else Interval.exact(se.z)
    ref, S, slack = BS.se_reduce_terms(se.gs, aiv, se.HW)
    iv = IV.sum_interval(ref, S, se.HW, R + splits, 1, slack).mul(BS.sig1m_interval(se.u), 1)
    a = emu_act(se.z, se.s, se.t, False) if virt else se.z
    _ok(IV.check_interval(_emu_se_reduce(se, a), iv, "se_bwd_reduce", None))
    for fault in ("drop_chunk_last", "double_split_first", "acc_bf16"):
        _rejected(lambda: IV.check_interval(_emu_se_reduce(se, a, fault), iv, "se_bwd_reduce " + fault, None))


def test_se_bwd_apply_emulation_and_faults(se):
    iv = BS.se_apply_interval(se.gs, se.u, se.dz, se.HW)
    dz4 = se.dz.view(se.N, 1, 1, se.C)
    inv = torch.tensor(1.0) / torch.tensor(float(se.HW))
    for end in (-1, 0, 1):
        _ok(IV.check_store_bound(bf16r(se.gs * se.sg(end) + dz4 * inv), iv, "se_bwd_apply end %d" % end, None))
    _rejected(lambda: IV.check_store_bound(bf16r(se.gs * se.sg() + dz4 / (se.HW + 1)), iv, "se_bwd_apply dz/(HW+1)", None))
    _rejected(lambda: IV.check_store_bound(bf16r(se.gs * se.sg()), iv, "se_bwd_apply without dz", None))


def _emu_proj(wp, N, kseg, W, u, fault=None):
    Co, Ci = W.shape
    wp = wp.view(N, kseg, Co, Ci)
    p = wp[:, 0].clone()
    for j in range(1, kseg - (1 if fault == "slab_dropped" else 0)):
        p = p + wp[:, j]
    acc = torch.zeros(N, Ci)
    for o in range(Co):
        acc = acc + W[o] * p[:, o]
    sg = _sig(u)
    du = acc * sg * (1.0 - sg)
    sgw = sg.clone()
    if fault == "sigma_last_image":
        sgw[N - 1] = 1.0
    dW = torch.zeros(Co, Ci)
    for n in range(N):
        dW = dW + p[n] * sgw[n]
    return du, dW


@pytest.mark.parametrize("N,kseg,Co,Ci", [(3, 4, 16, 48), (1, 1, 24, 72), (2, 2, 40, 264)])
def test_se_proj_finalize_emulation_and_faults(N, kseg, Co, Ci):
    wp = _u((N * kseg, Co, Ci), 41) * 5
    W, u = _u((Co, Ci), 42) * 0.3, 2 * _u((N, Ci), 43)
    du_iv, ref, S, slack, M = BS.se_proj_finalize_intervals(wp, N, kseg, W, u)
    du, dW = _emu_proj(wp, N, kseg, W, u)
    _ok(IV.check_interval(du, du_iv, "se_proj du", None))
    _ok(check_sum_bound(dW, ref, S, M, 0, 2, "se_proj dW", slack, family=None))
    if kseg > 1:
        du, dW = _emu_proj(wp, N, kseg, W, u, "slab_dropped")
        _rejected(lambda: IV.check_interval(du, du_iv, "se_proj du, slab dropped", None))
        _rejected(lambda: check_sum_bound(dW, ref, S, M, 0, 2, "se_proj dW, slab dropped", slack, family=None))
    _, dW = _emu_proj(wp, N, kseg, W, u, "sigma_last_image")
    _rejected(lambda: check_sum_bound(dW, ref, S, M, 0, 2, "se_proj dW without the last image's sigma", slack, family=None))


@pytest.mark.parametrize("N,E,R", [(5, 240, 10), (7, 100, 13), (2, 8, 1)])
def test_se_fc_emulation_and_faults(N, E, R):
    z = torch.rand(N, E, generator=torch.Generator().manual_seed(51))
    W1, b1 = torch.randn(R, E, generator=torch.Generator().manual_seed(52)) / E ** 0.5, 0.1 * _u((R,), 53) + 0.3
    W2, b2 = torch.randn(E, R, generator=torch.Generator().manual_seed(54)) / R ** 0.5, 0.1 * _u((E,), 55)
    du = _u((N, E), 56)
    hb_iv, u_iv, gate_iv = BS.se_fc_fwd_intervals(z, W1, b1, W2, b2)
    hb = torch.relu(z @ W1.t() + b1)
    u = hb @ W2.t() + b2
    _ok(IV.check_interval(hb, hb_iv, "se_fc hb", None))
    _ok(IV.check_interval(u, u_iv, "se_fc u", None))
    _ok(IV.check_interval(_sig(u), gate_iv, "se_fc gate", None))
    if R % 4:
        _rejected(lambda: IV.check_interval(hb[:, :R - 1] @ W2[:, :R - 1].t() + b2, u_iv, "se_fc u, last hidden unit dropped", None))
    base = {k: 0.5 * _u(s_, 60 + i) for i, (k, s_) in enumerate((("dW1", (R, E)), ("db1", (R,)), ("dW2", (E, R)), ("db2", (E,))))}
    for acc in (False, True):
        dh_iv, dz_iv, terms = BS.se_fc_bwd_terms(du, z, hb, W1, W2, base if acc else None)
        dh = (du @ W2) * (hb > 0)
        _ok(IV.check_interval(dh, dh_iv, "se_fc dh", None))
        _ok(IV.check_interval(dh @ W1, dz_iv, "se_fc dz", None))
        got = {"dW1": dh.t() @ z, "db1": dh.sum(0), "dW2": du.t() @ hb, "db2": du.sum(0)}
        for k, (ref, S, slack, c) in terms.items():
            _ok(check_sum_bound(got[k] + (base[k] if acc else 0), ref, S, N, 16, c, "se_fc " + k, slack, family=None))
        ref, S, slack, c = terms["dW1"]
        if acc:
            _rejected(lambda: check_sum_bound(got["dW1"], ref, S, N, 16, c, "se_fc dW1, accumulate ignored", slack, family=None))
        else:
            _rejected(lambda: check_sum_bound(dh[:N - 1].t() @ z[:N - 1], ref, S, N, 16, c, "se_fc dW1, last image dropped", slack, family=None))


# ---- stem -----------------------------------------------------------------------------------------------------------------------
def _emu_stem_wgrad(x, dy, fault=None, rb=4):
    """x (N,H,W,3), dy (N,Ho,Wo,Co) bf16 values -> (Co,3,3,3), fp32 accumulate"""
    N, H, W, _ = x.shape
    _, Ho, Wo, Co = dy.shape
    if fault == "right_column":
        x = x.clone()
        x[:, :, W - 1] = 0
    if fault == "last_band_row" and Ho % rb:
        dy = dy.clone()
        dy[:, Ho - 1] = 0
    xp = pad_hw(x, 1)
    if fault == "pad_replicated":
        xp[:, 0], xp[:, -1] = xp[:, 1], xp[:, -2]
        xp[:, :, 0], xp[:, :, -1] = xp[:, :, 1], xp[:, :, -2]
    dw = torch.zeros(Co, 3, 3, 3)
    d2 = dy.reshape(-1, Co)
    for kh in range(3):
        for kw in range(3):
            sl = xp[:, kh:kh + 2 * (Ho - 1) + 1:2, kw:kw + 2 * (Wo - 1) + 1:2]
            dw[:, :, kh, kw] = d2.t() @ sl.reshape(-1, 3)
    return dw


def test_stem_wgrad_emulation_and_faults():
    N, H, W, Co = 2, 20, 32, 32
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert BS.stem_wgrad_band_rows(W, Wo) == 4 and Ho % 4
    x = bf16r(_u((N, H, W, 3), 71))
    cf = _coefs(Co, 72)
    g, y = bf16r(_u((N, Ho, Wo, Co), 73)), off_hinge(bf16r(_u((N, Ho, Wo, Co), 74)), cf[0], cf[1])
    div = dy_interval(g, y, cf, bf16=True)
    ref, S, slack = wgrad_terms(Interval.exact(x), div, 3, 2, 1)
    dy = emu_dy(g, y, cf, True)
    M, P = N * Ho * Wo, 4
    _ok(check_sum_bound(_emu_stem_wgrad(x, dy), ref, S, M, P, 1, "stem wgrad", slack, family=None))
    for fault in ("right_column", "pad_replicated", "last_band_row"):
        _rejected(lambda: check_sum_bound(_emu_stem_wgrad(x, dy, fault), ref, S, M, P, 1, "stem wgrad " + fault, slack, family=None))


def _emu_stem_dgrad(dy, w, H, W, aff=None, fault=None):
    """dy (N,Ho,Wo,Co) bf16 values, w (Co,3,3,3) fp32 (rounded to bf16 here, as the kernel does) -> (N,3,H,W) fp32"""
    N, Ho, Wo, Co = dy.shape
    wb = w if fault == "weights_fp32" else bf16r(w)
    if fault == "last_row" and H % 2:
        dy = dy.clone()
        dy[:, Ho - 1] = 0
    gp = torch.zeros(N, max(H + 2, 2 * Ho + 1), max(W + 2, 2 * Wo + 1), 3)
    for kh in range(3):
        for kw in range(3):
            gp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += dy @ wb[:, :, kh, kw]
    dx = gp[:, 1:1 + H, 1:1 + W].permute(0, 3, 1, 2)
    if aff is not None:
        sc = aff[0].roll(1) if fault == "affine_plane" else aff[0]
        dx = dx * sc.view(1, 3, 1, 1)
    return dx.contiguous()


@pytest.mark.parametrize("Co", [8, 128])
def test_stem_dgrad_emulation_and_faults(Co):
    N, H, W = 2, 9, 11
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    cf = _coefs(Co, 75)
    g, y = bf16r(_u((N, Ho, Wo, Co), 76)), off_hinge(bf16r(_u((N, Ho, Wo, Co), 77)), cf[0], cf[1])
    w = _u((Co, 3, 3, 3), 78) * (1.0 / 27) ** 0.5
    assert not torch.equal(w, bf16r(w))
    aff = torch.tensor([[2.0, 0.5, 1.25], [0.1, 0.2, 0.3]])
    div = dy_interval(g, y, cf, bf16=True)
    dy = emu_dy(g, y, cf, True)
    for a_ in (None, aff):
        ref, bound = BS.stem_dgrad_terms(div, bf16r(w), H, W, a_)
        _ok(IV._assert_bound(_emu_stem_dgrad(dy, w, H, W, a_), ref, bound, "stem dgrad", None))
        for fault in ("last_row", "weights_fp32") + (("affine_plane",) if a_ is not None else ()):
            _rejected(lambda: IV._assert_bound(_emu_stem_dgrad(dy, w, H, W, a_, fault), ref, bound, "stem dgrad " + fault, None))


# ---- glue -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,HW,C_", [(2, 49, 320), (1, 1, 8), (3, 9, 8)])
@pytest.mark.parametrize("virt", [True, False])
def test_pool_act_emulation_and_faults(N, HW, C_, virt):
    x = bf16r(_u((N, HW, C_), 81))
    s, t = 1 + 0.3 * _u((C_,), 82), 0.2 * _u((C_,), 83)
    aiv = act_interval(x, s, t, bf16=False) if virt else Interval.exact(x)
    ref, bound = BS.pool_act_terms(aiv, HW)
    a = emu_act(x, s, t, False) if virt else x
    R = 256 // (C_ // 8)
    acc = torch.zeros(N, C_)
    for p in range(HW):
        acc = acc + a[:, p]
    _ok(IV._assert_bound(acc / HW, ref, bound, "pool_act", None))
    padded = -(-HW // (8 * R)) * 8 * R
    _rejected(lambda: IV._assert_bound(acc / padded, ref, bound, "pool_act / padded count", None))
    if HW > 1:
        _rejected(lambda: IV._assert_bound((acc - a[:, HW - 1]) / HW, ref, bound, "pool_act, last pixel dropped", None))


def test_add_act_emulation_and_faults():
    rows, C_ = 98, 320
    a, b = bf16r(_u((rows, C_), 84)), bf16r(_u((rows, C_), 85))
    sa, ta, sb, tb = 1 + 0.3 * _u((C_,), 86), 0.2 * _u((C_,), 87), 1 + 0.3 * _u((C_,), 88), 0.2 * _u((C_,), 89)
    iv = BS.add_act_interval(act_interval(a, sa, ta, bf16=False), act_interval(b, sb, tb, bf16=False))
    v = emu_act(a, sa, ta, False) + emu_act(b, sb, tb, False)
    _ok(IV.check_interval(v, iv, "add_act fp32", None))
    _ok(IV.check_store_bound(bf16r(v), iv, "add_act bf16", None))
    _rejected(lambda: IV.check_interval(bf16r(emu_act(a, sa, ta, False)) + emu_act(b, sb, tb, False), iv, "add_act: a rounded to bf16", None))
    _rejected(lambda: IV.check_store_bound(bf16r(bf16r(emu_act(a, sa, ta, False)) + emu_act(b, sb, tb, False)), iv, "add_act bf16: two roundings", None))


# ---- finalizes ------------------------------------------------------------------------------------------------------------------
def _emu_bn_fwd(partial, count, gamma, beta, rm, rv, mom=0.1, eps=1e-5, fault=None):
    """k_bn_fwd_finalize: fp32 partial sums per accumulator (exact here: T = 1), then double, one fp32 rounding per output"""
    dt = torch.float32 if fault == "fp32" else torch.float64
    mom, eps = torch.tensor(mom, dtype=torch.float32).to(dt), torch.tensor(eps, dtype=torch.float32).to(dt)
    s1, s2 = partial[0].double().sum(-1).to(dt), partial[1].double().sum(-1).to(dt)
    cnt = torch.tensor(count, dtype=dt)
    mean = s1 / cnt
    var = s2 / cnt - mean * mean
    if fault != "no_clamp":
        var = var.clamp_min(0)
    invstd = 1 / torch.sqrt(var + eps)
    g, b = gamma.to(dt), beta.to(dt)
    unb = var if (count <= 1 or fault == "biased") else var * cnt / (cnt - 1)
    return {"s": g * invstd, "t": b - mean * g * invstd, "mean": mean, "invstd": invstd,
            "running_mean": (1 - mom) * rm.to(dt) + mom * mean, "running_var": (1 - mom) * rv.to(dt) + mom * unb}


@pytest.mark.parametrize("C_,nparts,count", [(16, 7, 100.0), (8, 256, 50176.0), (8, 1024, 802816.0), (8, 1, 1.0), (8, 1, 64.0)])
def test_bn_fwd_finalize_emulation_and_faults(C_, nparts, count):
    Ct = C_ + 3
    partial = BS.bn_fwd_partials(_u((2, Ct, nparts), 91), count)
    gamma, beta = 1 + 0.2 * _u((Ct,), 92), 0.1 * _u((Ct,), 93)
    rm, rv = 0.1 * _u((Ct,), 94), 1 + 0.3 * _u((Ct,), 95).abs()
    ivs = BS.bn_fwd_finalize_intervals(partial, count, gamma, beta, rm, rv, 0.1, 1e-5)
    got = _emu_bn_fwd(partial, count, gamma, beta, rm, rv)
    for k, iv in ivs.items():
        _ok(IV.check_interval(got[k].float(), iv, "bn_fwd_finalize " + k, None))
    assert float(ivs["invstd"].half[-1]) < 1e-6 * float(ivs["invstd"].mid[-1])          # the clamped channel: both ends at var = 0
    bad = _emu_bn_fwd(partial, count, gamma, beta, rm, rv, fault="fp32")
    if count > 1:
        ch = Ct - 3                                                                       # |mean|/std = 30
        one = Interval(ivs["invstd"].lo[ch], ivs["invstd"].hi[ch])
        _rejected(lambda: IV.check_interval(bad["invstd"][ch].float(), one, "bn_fwd_finalize in fp32 at |mean|/std = 30", None))
        bad = _emu_bn_fwd(partial, count, gamma, beta, rm, rv, fault="biased")
        _rejected(lambda: IV.check_interval(bad["running_var"].float(), ivs["running_var"], "biased variance into running_var", None))
        bad = _emu_bn_fwd(partial, count, gamma, beta, rm, rv, fault="no_clamp")
        _rejected(lambda: IV.check_interval(bad["invstd"].float(), ivs["invstd"], "no clamp on a negative var", None))


@pytest.mark.parametrize("nparts", [7, 257, 1025])
def test_bn_bwd_finalize_emulation_and_faults(nparts):
    C_, count = 24, 12345.0
    partial = _u((2, C_, nparts), 96)
    bn = _coefs(C_, 97)
    g0, b0, c0 = _u((C_,), 98), _u((C_,), 99), _u((C_,), 100)

    def emu(fault=None):
        s1, s2 = partial[0].double().sum(-1), partial[1].double().sum(-1)
        s, mean, inv = bn[0].double(), bn[5].double(), bn[6].double()
        cnt = count - 1 if fault == "count" else count
        c3 = s * (mean * inv * s2 / cnt - s1 / cnt)
        return {"c1": s.float(), "c2": (-s * inv * s2 / cnt).float(), "c3": (-c3 if fault == "sign" else c3).float(),
                "dgamma": g0 + s2.float(), "dbeta": b0 + s1.float(), "dbias": c0 + (s * s1).float()}
    ivs = BS.bn_bwd_finalize_intervals(partial, count, bn, g0, b0)
    ivs["dbias"] = BS.bn_bwd_finalize_intervals(partial, count, bn, g0, b0, frozen=True, dbias0=c0)["dbias"]
    got = emu()
    for k, iv in ivs.items():
        _ok(IV.check_interval(got[k], iv, "bn_bwd_finalize " + k, None))
    _rejected(lambda: IV.check_interval(emu("sign")["c3"], ivs["c3"], "bn_bwd_finalize: sign of row 4", None))
    if nparts <= 1024:          # (at T = 2 the bracket of the fp32 partial sums is wider than 1/count)
        _rejected(lambda: IV.check_interval(emu("count")["c2"], ivs["c2"], "bn_bwd_finalize: count - 1", None))
    _rejected(lambda: IV.check_interval(got["dgamma"] - g0, ivs["dgamma"], "bn_bwd_finalize: accumulate ignored", None))


@pytest.mark.parametrize("nsplit,acc", [(5, 0), (300, 1), (129, 1)])
def test_wgrad_finalize_emulation_and_faults(nsplit, acc):
    part, init = _u((nsplit, 24, 16), 101), _u((24, 16), 102)
    ref = part.double().sum(0) + (init.double() if acc else 0)
    S = part.double().abs().sum(0) + (init.double().abs() if acc else 0)
    got = torch.zeros(24, 16)
    for p in range(nsplit):
        got = got + part[p]
    _ok(check_sum_bound(got + (init if acc else 0), ref, S, nsplit, 0, 1, "wgrad finalize", None, family=None))
    _rejected(lambda: check_sum_bound(got - part[nsplit - 1] + (init if acc else 0), ref, S, nsplit, 0, 1, "wgrad finalize, last split dropped", None, family=None))
    if acc:
        _rejected(lambda: check_sum_bound(got, ref, S, nsplit, 0, 1, "wgrad finalize, accumulate ignored", None, family=None))


# ---- the condition of the gated MFMA operand, known to hold before anything runs on a GPU ------------------------------------------
@pytest.mark.parametrize("shape", [(2, 16, 9, 48, 16), (9, 28, 28, 240, 40)])
def test_gated_operand_straddle_share_of_the_gpu_tests(shape):
    """the inputs of tests/test_gpu_se.py::test_gated_project_forward where it asserts check_onload_bound over
    gated_act_interval(..., bf16=True): the share of bf16 elements whose bracket straddles a rounding boundary is <= MAX_ACT_SPLIT"""
    from cases import O
    y, s, t, u, w, bias = BS.gated_fwd_inputs(shape, O)
    yn = y.permute(0, 2, 3, 1)
    iv = BS.gated_act_interval(yn, s, t, BS.gate_nhwc(BS.sigmoid_interval(u), yn.shape), bf16=True)
    print("gated operand %s: straddle share %.3g" % (shape, iv.split_share()))
    assert iv.split_share() <= BC.MAX_ACT_SPLIT


# ---- the fp32 tail of the step: head GEMMs, cross-entropy, optimizers ----------------------------------------------------------------
# fp32 torch arithmetic in the kernels' operation order; `fused` swaps every multiply-and-add a compiler may contract (and the
# source's own fmaf) between one rounding (through fp64: a product of two fp32 numbers is exact there) and two.
def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _trunc10(t):
    return (t.contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)


def emu_head_gemm(A, B, bias=None, C0=None, relu=False, post=None, mask_src=None, fused=True, fault=None):
    """k_head_gemm: wave w of 8 takes k = 128 t + 16 w + j of every K step t, the eight partial tiles are added in wave order"""
    M, K = A.shape
    N = B.shape[1]
    if fault == "operand_bf16":
        A, B = bf16r(A), bf16r(B)
    if fault == "trunc10":
        A, B = _trunc10(A), _trunc10(B)
    T = -(-K // 128)
    Ap, Bp = torch.zeros(M, T * 128), torch.zeros(T * 128, N)
    Ap[:, :K], Bp[:K] = A, B
    acc = torch.zeros(8, M, N)
    for t in range(T):
        for j in range(16):
            ks = t * 128 + torch.arange(8) * 16 + j
            a, b = Ap[:, ks].t()[:, :, None], Bp[ks][:, None, :]
            acc = _fma(a, b, acc) if fused else acc + a * b
    v = torch.zeros(M, N)
    for w in range(8):
        v = bf16r(v + acc[w]) if fault == "partials_bf16" else v + acc[w]
    if bias is not None:
        b = bias.clone()
        if fault == "bias_missing":
            b[int(b.abs().argmax())] = 0.0
        v = v + b
    if relu:
        v = torch.relu(v)
    if post is not None:
        v = v * post
    if mask_src is not None:
        v = v * ((mask_src >= 0) if fault == "mask_ge" else (mask_src > 0))
    return v if C0 is None else C0 + v


def emu_head_rowsum(A, r0=None):
    M, K = A.shape
    T = -(-K // 128)
    Ap = torch.zeros(M, T * 128)
    Ap[:, :K] = A
    s = torch.zeros(8, M)
    for t in range(T):
        for j in range(0, 16, 4):
            ks = t * 128 + torch.arange(8)[:, None] * 16 + j + torch.arange(4)[None, :]
            a = Ap[:, ks]                                        # (M, 8, 4)
            s = s + ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])).t()
    v = torch.zeros(M)
    for w in range(8):
        v = v + s[w]
    return v if r0 is None else r0 + v


def _head_case(N, I, O_, p, scaled):
    x, w, b, dz, u_prev, c0w, c0b = BT.head_inputs(N, I, O_, scaled)
    keep = (_u((N, I), 99) > 2 * p - 1) if p else torch.ones(N, I, dtype=torch.bool)
    xd = BT.head_dropped(x, keep, p)
    post = keep * BT.head_drop_scale(p) if p else None
    return x, w, b, dz, u_prev, c0w, c0b, keep, xd, post


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("N,I,O_", [(5, 512, 10), (130, 70, 65), (1, 1, 1), (1, 129, 1), (33, 128, 33), (32, 127, 32)])
def test_head_gemm_emulations_inside_bound(N, I, O_, scaled):
    for p in (0.0, 0.5, 0.999):
        x, w, b, dz, u_prev, c0w, c0b, keep, xd, post = _head_case(N, I, O_, p, scaled)
        for fused in (True, False):
            for relu in (False, True):
                _ok(IV.check_interval(emu_head_gemm(xd, w.t(), b, relu=relu, fused=fused),
                                     BT.head_gemm_interval(xd, w.t(), b, relu=relu), "head fwd", None))
            _ok(IV.check_interval(emu_head_gemm(xd, w.t(), fused=fused), BT.head_gemm_interval(xd, w.t()), "head fwd, no bias", None))
            _ok(IV.check_interval(emu_head_gemm(dz.t(), xd, C0=c0w, fused=fused), BT.head_gemm_interval(dz.t(), xd, C0=c0w), "head dW", None))
            mask = u_prev > 0
            _ok(IV.check_interval(emu_head_gemm(dz, w, post=post, mask_src=u_prev, fused=fused),
                                 BT.head_gemm_interval(dz, w, post=post, mask=mask), "head dx", None))
        _ok(IV.check_interval(emu_head_rowsum(dz.t(), c0b), BT.head_rowsum_interval(dz.t(), c0b), "head db", None))


@pytest.mark.parametrize("fault", ["operand_bf16", "trunc10", "partials_bf16", "bias_missing", "mask_ge"])
@pytest.mark.parametrize("N,I,O_", [(130, 70, 65), (33, 128, 33)])
def test_head_gemm_faults_rejected(N, I, O_, fault):
    x, w, b, dz, u_prev, c0w, c0b, keep, xd, post = _head_case(N, I, O_, 0.2, True)
    if fault == "mask_ge":
        iv = BT.head_gemm_interval(dz, w, post=post, mask=u_prev > 0)
        _rejected(lambda: IV.check_interval(emu_head_gemm(dz, w, post=post, mask_src=u_prev, fault=fault), iv, "head dx " + fault, None))
        return
    iv = BT.head_gemm_interval(xd, w.t(), b)
    _rejected(lambda: IV.check_interval(emu_head_gemm(xd, w.t(), b, fault=fault), iv, "head fwd " + fault, None))
    if fault != "bias_missing":
        iv = BT.head_gemm_interval(dz.t(), xd, C0=c0w)
        _rejected(lambda: IV.check_interval(emu_head_gemm(dz.t(), xd, C0=c0w, fault=fault), iv, "head dW " + fault, None))


def test_head_sparse_probe_sees_a_dropped_and_a_doubled_term():
    N, I, O_ = 130, 133, 131
    x, w, b, dz, u_prev, c0w, c0b = BT.head_inputs(N, I, O_, False)
    cases = {"fwd": (BT.head_sparse(x, 1, I), w.t()), "dW": (BT.head_sparse(dz.t(), 1, N), x), "dx": (BT.head_sparse(dz, 1, O_), w)}
    for name, (A, B) in cases.items():
        iv = BT.head_gemm_interval(A, B)
        BT.head_probe_visible(A, B, iv, name)
        _ok(IV.check_interval(emu_head_gemm(A, B), iv, "sparse " + name, None))
        for k in BT.HEAD_LIVE_K(A.shape[1]):
            for f in (0.0, 2.0):
                A2 = A.clone()
                A2[:, k] *= f
                _rejected(lambda: IV.check_interval(emu_head_gemm(A2, B), iv, "sparse %s k %d x%g" % (name, k, f), None))
    A = BT.head_sparse(dz.t(), 1, N)
    iv = BT.head_rowsum_interval(A)
    _ok(IV.check_interval(emu_head_rowsum(A), iv, "sparse db", None))
    for k in BT.HEAD_LIVE_K(N):
        A2 = A.clone()
        A2[:, k] = 0
        _rejected(lambda: IV.check_interval(emu_head_rowsum(A2), iv, "sparse db k %d dropped" % k, None))


def _wg_sum(v):
    """head_wg_reduce over the last dimension: lane t of 256 adds elements t, t + 256, ... in order, a 64-lane xor butterfly, then
    ((w0 + w1) + w2) + w3"""
    n = v.shape[-1]
    T = -(-n // 256)
    pad = torch.zeros(v.shape[:-1] + (T * 256,), dtype=v.dtype)
    pad[..., :n] = v
    pad = pad.view(v.shape[:-1] + (T, 256))
    s = torch.zeros(v.shape[:-1] + (256,), dtype=v.dtype)
    for t in range(T):
        s = s + pad[..., t, :]
    s = s.view(v.shape[:-1] + (4, 64))
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    r = s[..., 0]
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def emu_ce(x, ta, tb=None, lam=None, eps=None, fused=False, fault=None, ignore_index=-100):
    """k_head_ce (eps None) / k_head_ce_soft and their mean stage -> (dlogits, loss_rows, loss)"""
    N, Cn = x.shape
    b = ta if tb is None else tb
    l = torch.ones(N) if (tb is None or lam is None) else lam.float()
    ignored = (ta == ignore_index) | (b == ignore_index)
    cnt = (~ignored).float().sum()
    a0, b0 = torch.where(ignored, torch.zeros_like(ta), ta), torch.where(ignored, torch.zeros_like(b), b)
    rowi = torch.arange(N)
    mx = x.max(1, keepdim=True).values
    e = torch.exp(x - mx)
    es = e.clone()
    if fault == "se_skips_last" and Cn % 256 == 1:
        es[:, -1] = 0.0
    se = _wg_sum(es)[:, None]
    rse = 1.0 / se
    inv = torch.where(ignored, torch.zeros(N), 1.0 / (torch.tensor(float(N)) if fault == "grad_div_N" else cnt))[:, None]
    ep = torch.tensor(0.0 if eps is None else eps, dtype=torch.float32)
    same = ta == b
    if eps is None:
        wa, wb, u = torch.ones(N), torch.zeros(N), torch.tensor(0.0)
    else:
        ome = 1.0 - ep
        wa = torch.where(same, ome.expand(N), ome * l)
        wb = torch.where(same, torch.zeros(N), _fma(-ome.expand(N), l, ome.expand(N)) if fused else ome - wa)
        if fault == "wb_on_same":
            wb = torch.where(same, ome * (1.0 - l), wb)
        u = ep / float(Cn)
    qa, qb = torch.zeros(N, Cn), torch.zeros(N, Cn)
    qa[rowi, a0] = wa
    nb = ~same if fault != "wb_on_same" else torch.ones(N, dtype=torch.bool)
    qb[rowi[nb], b0[nb]] = wb[nb]
    q = (qa + qb) + u
    if fault == "u_missing_at_labels":
        q[rowi, a0] = (qa + qb)[rowi, a0]
        q[rowi, b0] = (qa + qb)[rowi, b0]
    if fault == "p_bf16":
        d = bf16r(e * rse) - q
    else:
        d = _fma(e, rse.expand_as(e), -q) if fused else e * rse - q
    dl = torch.where(ignored[:, None], torch.zeros(N, Cn), d * inv)
    lse = torch.log(se[:, 0]) + mx[:, 0]
    za, zb = x[rowi, a0], x[rowi, b0]
    if eps is None:
        rows = lse - za
    else:
        t1, t2 = lse - za, lse - zb
        r = _fma(wb, t2, wa * t1) if fused else wa * t1 + wb * t2
        if float(ep) != 0.0:
            t3 = lse - _wg_sum(x) / float(Cn)
            r = _fma(ep.expand(N), t3, r) if fused else r + ep * t3
        rows = r
    rows = torch.where(ignored, torch.zeros(N), rows)
    loss = _wg_sum(rows) / (torch.tensor(float(N)) if fault == "mean_over_N" else cnt)
    return dl, rows, loss


def _ce_check(x, ta, tb, lam, eps, fused=False, fault=None):
    dl, rows, loss = emu_ce(x, ta, tb, lam, eps, fused, fault)
    iv = BT.ce_intervals(x, ta, tb, lam, eps)
    r = [IV.check_interval(dl, iv["dl"], "ce dlogits", None), IV.check_interval(rows, iv["rows"], "ce loss rows", None)]
    r.append(BT.check_ce_mean(loss, rows, iv["count"], "ce mean", None))
    if iv["count"] == 0:
        assert bool((dl == 0).all())
    return max(r)


def _soft_args(N, Cn, how):
    a, b = BT.ce_targets(N, Cn)
    lam = torch.tensor([0.0, 0.5, 1.0, 0.3, 0.8125, 0.49999997])[torch.arange(N) % 6]
    b = torch.where(torch.arange(N) % 4 == 1, a, b)                      # rows with a == b among the others
    return BT.ce_ignore(a, how), b, lam


@pytest.mark.parametrize("N,Cn", BT.CE_SIZES)
def test_cross_entropy_emulations_inside_bracket(N, Cn):
    worst = 0.0
    for i, kind in enumerate(BT.CE_ROWS):
        x = BT.ce_logits(kind, N, Cn)
        for how in (BT.CE_IGNORE if N * Cn <= 10000 else BT.CE_IGNORE[i % 4:i % 4 + 1]):
            a, b, lam = _soft_args(N, Cn, how)
            for fused in (False, True):
                worst = max(worst, _ce_check(x, a, None, None, None, fused))
                for eps in (0.0, 0.1, 1.0):
                    worst = max(worst, _ce_check(x, a, b, lam, eps, fused), _ce_check(x, a, None, None, eps, fused))
    print("N %d C %d: worst emulation / bracket %.3f" % (N, Cn, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("fault,N,Cn,how,eps", [("grad_div_N", 257, 10, "third", None), ("grad_div_N", 7, 255, "all_but_one", 0.1),
                                                ("mean_over_N", 257, 10, "third", None), ("mean_over_N", 7, 255, "third", 0.1),
                                                ("u_missing_at_labels", 7, 255, "none", 0.1), ("u_missing_at_labels", 257, 10, "third", 1.0),
                                                ("se_skips_last", 7, 513, "none", None), ("se_skips_last", 7, 513, "none", 0.1),
                                                ("p_bf16", 7, 256, "none", None), ("p_bf16", 257, 10, "third", 0.1),
                                                ("wb_on_same", 7, 255, "none", 0.1), ("wb_on_same", 257, 10, "third", 0.0)])
def test_cross_entropy_faults_rejected(fault, N, Cn, how, eps):
    """wb_on_same: the label of a row with a == b gets wa = 1 - eps AND a share wb on top.  (The milder variant -- such a row
    treated as any other, two rounded shares that add up to 1 - eps within one ulp -- moves q by at most u and lies inside any
    bracket that allows the kernel's own roundings of p - q: it cannot be separated and is not claimed.)"""
    x = BT.ce_logits("uniform4", N, Cn)
    a, b, lam = _soft_args(N, Cn, how)
    tb, l = (None, None) if eps is None else (b, lam)
    _ok(_ce_check(x, a, tb, l, eps))
    _rejected(lambda: _ce_check(x, a, tb, l, eps, fault=fault))


def _opt_state(n):
    return BT.opt_data(n, seed=n)


def emu_adam(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, coef=None, fused=False, fault=None):
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    lr, b1, b2, eps, wd, gscale = (f(c) for c in (lr, b1, b2, eps, wd, gscale))
    bc1, bc2s = (f(c) for c in BT.adam_bias(float(b1), float(b2), step))
    gi = g * gscale
    if coef is not None:
        gi = gi * f(coef)
    if float(wd) != 0.0 and fault != "decoupled_wd":
        gi = _fma(wd.expand_as(p), p, gi)
    mi = _fma(b1.expand_as(m), m, (1.0 - b1) * gi)
    gv = gi * gscale if fault == "gscale_twice_v" else gi
    vi = _fma(b2.expand_as(v), v, (1.0 - b2) * gv * gv)
    if fault == "v_bf16":
        vi = bf16r(vi)
    if fault == "eps_in_sqrt":
        denom = torch.sqrt(vi + eps) / bc2s
    elif fault == "no_bc2":
        denom = torch.sqrt(vi) + eps
    else:
        denom = torch.sqrt(vi) / bc2s + eps
    ss, r = lr / bc1, mi / denom
    pn = _fma(-ss.expand_as(p), r, p) if fused else p - ss * r
    if fault == "decoupled_wd":
        pn = pn - lr * wd * p
    return dict(p=pn, m=mi, v=vi)


def emu_rmsprop(p, g, sq, buf, lr, alpha, eps, wd, momentum, gscale, fused=False, fault=None):
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    lr, alpha, eps, wd, momentum, gscale = (f(c) for c in (lr, alpha, eps, wd, momentum, gscale))
    gi = g * gscale
    if float(wd) != 0.0:
        gi = _fma(wd.expand_as(p), p, gi)
    s = _fma(alpha.expand_as(sq), sq, (1.0 - alpha) * gi * gi)
    if fault == "v_bf16":
        s = bf16r(s)
    avg = torch.sqrt(s + eps) if fault == "eps_in_sqrt" else torch.sqrt(s) + eps
    r = gi / avg
    out = dict(sq=s)
    if float(momentum) > 0:
        r = _fma(momentum.expand_as(buf), buf, r)
        out["buf"] = r
    out["p"] = _fma(-lr.expand_as(p), r, p) if fused else p - lr * r
    return out


def emu_sgd(p, g, buf, lr, momentum, dampening, wd, nesterov, step, gscale, fused=False, fault=None):
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    lr, momentum, dampening, wd, gscale = (f(c) for c in (lr, momentum, dampening, wd, gscale))
    gi = g * gscale
    if float(wd) != 0.0:
        gi = _fma(wd.expand_as(p), p, gi)
    out = {}
    if float(momentum) != 0.0:
        if step == 1 and fault != "damp_first":
            b = gi
        elif step == 1:
            b = (1.0 - dampening) * gi
        else:
            b = _fma(momentum.expand_as(buf), buf, (1.0 - dampening) * gi)
        out["buf"] = b
        gi = _fma(momentum.expand_as(b), b, gi) if (nesterov and fault != "no_nesterov") else b
    out["p"] = _fma(-lr.expand_as(p), gi, p) if fused else p - lr * gi
    return out


def _opt_check(got, ivs, what):
    return max(_ok(IV.check_interval(got[k], ivs[k], "%s %s" % (what, k), None)) for k in ivs)


ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_optimizer_emulations_inside_bracket(n):
    p, g, m, v, buf = _opt_state(n)
    for fused in (False, True):
        for step in (1, 2, 1000, 100000):
            for wd in (0.0, 1e-2):
                for gs in (1.0, 0.125, 1.0 / 3):
                    _opt_check(emu_adam(p, g, m, v, wd=wd, step=step, gscale=gs, fused=fused, **ADAM),
                               BT.adam_intervals(p, g, m, v, wd=wd, step=step, gscale=gs, **ADAM), "adam")
        _opt_check(emu_adam(p, g, m, v, wd=1e-2, step=2, gscale=0.125, coef=0.37, fused=fused, **ADAM),
                   BT.adam_intervals(p, g, m, v, wd=1e-2, step=2, gscale=0.125, coef=Interval.exact(IV.f32(0.37)), **ADAM), "adam_ex")
        for mom in (0.0, 0.9):
            for wd in (0.0, 1e-2):
                a = dict(lr=1e-2, alpha=0.99, eps=1e-8, wd=wd, momentum=mom, gscale=1.0 / 3)
                _opt_check(emu_rmsprop(p, g, v, buf, fused=fused, **a), BT.rmsprop_intervals(p, g, v, buf, **a), "rmsprop")
            for damp in (0.0, 0.5):
                for nest in (0, 1):
                    for step in (1, 2):
                        if nest and (mom == 0.0 or damp != 0.0):
                            continue
                        a = dict(lr=1e-2, momentum=mom, dampening=damp, wd=1e-2, nesterov=nest, step=step, gscale=0.125)
                        _opt_check(emu_sgd(p, g, buf, fused=fused, **a), BT.sgd_intervals(p, g, buf, **a), "sgd")


@pytest.mark.parametrize("n", [255, 257])
@pytest.mark.parametrize("fault", ["v_bf16", "eps_in_sqrt", "no_bc2", "decoupled_wd", "gscale_twice_v"])
def test_adam_and_rmsprop_faults_rejected(n, fault):
    p, g, m, v, buf = _opt_state(n)
    a = dict(wd=1e-2, step=2, gscale=0.125, **ADAM)
    iv = BT.adam_intervals(p, g, m, v, **a)
    _rejected(lambda: _opt_check(emu_adam(p, g, m, v, fault=fault, **a), iv, "adam " + fault))
    if fault in ("v_bf16", "eps_in_sqrt"):
        a = dict(lr=1e-2, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.9, gscale=1.0)
        iv = BT.rmsprop_intervals(p, g, v, buf, **a)
        _rejected(lambda: _opt_check(emu_rmsprop(p, g, v, buf, fault=fault, **a), iv, "rmsprop " + fault))


@pytest.mark.parametrize("n", [255, 257])
@pytest.mark.parametrize("fault,step", [("damp_first", 1), ("no_nesterov", 1), ("no_nesterov", 2)])
def test_sgd_faults_rejected(n, fault, step):
    p, g, m, v, buf = _opt_state(n)
    nest = fault == "no_nesterov"
    a = dict(lr=1e-2, momentum=0.9, dampening=0.0 if nest else 0.5, wd=0.0, nesterov=int(nest), step=step, gscale=1.0)
    iv = BT.sgd_intervals(p, g, buf, **a)
    _opt_check(emu_sgd(p, g, buf, **a), iv, "sgd")
    _rejected(lambda: _opt_check(emu_sgd(p, g, buf, fault=fault, **a), iv, "sgd " + fault))


def test_ema_bound_and_the_old_p_fault():
    p, g, m, v, buf = _opt_state(257)
    ema = p * 0.9 + 0.01
    pn = emu_sgd(p, g, buf, lr=1e-2, momentum=0.0, dampening=0.0, wd=0.0, nesterov=0, step=1, gscale=1.0)["p"]
    for d in (0.0, 0.999):
        dd = torch.tensor(d, dtype=torch.float32)
        for fused in (False, True):
            got = _fma(dd.expand_as(ema), ema, (1.0 - dd) * pn) if fused else dd * ema + (1.0 - dd) * pn
            _ok(BT.check_ema(got, d, ema, pn, "ema", None))
        old = dd * ema + (1.0 - dd) * p
        _rejected(lambda: BT.check_ema(old, d, ema, pn, "ema from the old p", None))


# ---- the multi-label loss and HardDice (csrc/mnas_mlabel.hip) ---------------------------------------------------------------------------
# A numpy float32 emulation of k_mlabel_row in the kernel's lane order (scalar: lane l adds l, l + 256, ...; vector: the quads at
# 4 l + 1024 k, x y z w in turn), the 64-lane butterfly, ((w0 + w1) + w2) + w3; `fused` swaps `- z*t +` and `ls += e*w` between one
# rounding (through fp64: the product of two fp32 numbers is exact there) and two; the batch stage and the focal transform in
# float64, k_mlabel_scale as one fp32 product.
F32, F64 = np.float32, np.float64
ML_CAP = 4096 * 256


def _ml_order(C_, vec):
    T = BM.mlabel_trips(C_, vec)
    k, l = np.arange(T)[:, None], np.arange(256)[None, :]
    idx = 1024 * (k // 4) + 4 * l + k % 4 if vec else 256 * k + l
    return np.where(idx < C_, idx, -1)


def emu_mlabel(z, t, w, focal, gamma, balance, vec, fused, fault=None):
    """-> dict(dl, rows, loss, s) of torch tensors; every `fault` is one of the issue's list"""
    z, t = z.numpy().astype(F32), t.numpy().astype(F32)
    N, C_ = z.shape
    ww = np.ones_like(z) if w is None else w.numpy().astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        ea = np.exp(-np.abs(z))
        l1 = np.log(F32(1) + ea) if fault == "log_not_log1p" else np.log1p(ea)
        m = np.maximum(z, F32(0))
        A = (m.astype(F64) - z.astype(F64) * t.astype(F64)).astype(F32) if fused else m - z * t
        e = A + l1
        d = F32(1) + ea
        if fault == "other_sigmoid":
            sg = F32(1) / (F32(1) + np.exp(-z))
        else:
            sg = np.where(z >= 0, F32(1) / d, ea / d)
        inv = F32(1.0 / float(N)) if fault == "inv_N" else F32(BM.mlabel_inv(N, C_))
        df = sg - t
        dl = (ww * (ww * df)) * inv if fault == "w_twice" else df * inv if fault == "w_none" else (ww * df) * inv
    es, ws = e.copy(), ww
    if fault == "last_elem_dropped":
        es[:, -1] = 0
    if fault == "last_quad_dropped":
        es[:, -4:] = 0
    ls = np.zeros((N, 256), F32)
    for row in _ml_order(C_, vec):
        ok, ii = row >= 0, np.clip(row, 0, None)
        ev, wv = es[:, ii], ws[:, ii]
        new = (ls.astype(F64) + ev.astype(F64) * wv.astype(F64)).astype(F32) if fused else ls + ev * wv
        ls = np.where(ok[None, :], new, ls)
    s_ = ls.reshape(N, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s_ = s_ + s_[..., lane ^ o]
    r = s_[..., 0]
    rows = (r[:, 0] + r[:, 1]) + r[:, 3] if fault == "skip_wave" else ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]
    b = F32(rows.astype(F64).sum() / (float(N) if fault == "mean_N" else float(N) * float(C_)))
    loss, s = b, None
    if focal:
        bd, g, bal = F64(b), F64(F32(gamma)), F64(F32(balance))
        pt = np.exp(-bd)
        om = 1.0 - pt
        loss = F32(bal * np.power(om, g) * bd)
        s = F32(bal * np.power(om, g if fault == "focal_gamma_exp" else g - 1.0) * (om + g * pt * bd))
        flat = dl.reshape(-1)
        sc = flat * s
        if fault == "scale_none_beyond":
            sc[ML_CAP:] = flat[ML_CAP:]
        if fault == "scale_twice_beyond":
            sc[ML_CAP:] = sc[ML_CAP:] * s
        dl = sc.reshape(N, C_)
    tt = lambda v: None if v is None else torch.from_numpy(np.asarray(v, dtype=F32))
    return dict(dl=tt(dl), rows=tt(rows), loss=tt(loss), s=tt(s))


def _ml_check(z, t, w, focal, gamma, balance, vec, fused=False, fault=None, only=None):
    got = emu_mlabel(z, t, w, focal, gamma, balance, vec, fused, fault)
    N, C_ = z.shape
    iv = BM.mlabel_intervals(z, t, w, N, C_, focal, gamma, balance, vec, rows_dev=got["rows"])
    r = 0.0
    for k in ("dl", "rows", "loss", "s"):
        if got[k] is not None and (only is None or k in only):
            r = max(r, IV.check_interval(got[k], iv[k], "mlabel " + k, None))
    return r


ML_VARIANTS = (("plain", False, False), ("weighted", True, False), ("focal", False, True), ("weighted_focal", True, True))


@pytest.mark.parametrize("N,Cn", BM.ML_SHAPES)
def test_mlabel_emulations_inside_bracket(N, Cn):
    worst = 0.0
    for ki, kind in enumerate(BM.ML_KINDS):
        z, t, w = BM.mlabel_inputs(kind, N, Cn)
        gamma, balance = BM.ML_FOCAL[ki % 3]
        for name, weighted, focal in ML_VARIANTS:
            for vec in ((False, True) if Cn % 4 == 0 else (False,)):
                for fused in (False, True):
                    worst = max(worst, _ml_check(z, t, w if weighted else None, focal, gamma, balance, vec, fused))
        if kind == "sparse":
            BM.mlabel_probe_visible(BM.mlabel_intervals(z, t, w, N, Cn, False, 2.0, 0.25, Cn % 4 == 0), BM.mlabel_live(N, Cn), "sparse")
    print("N %d C %d: worst emulation / bracket %.3f" % (N, Cn, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("fault,N,Cn,kind,weighted,focal,vec,only", [
    ("last_elem_dropped", 3, 1027, "scale8", True, False, False, "rows"), ("last_elem_dropped", 2, 1000, "scale0.5", False, True, False, "rows"),
    ("last_quad_dropped", 3, 1028, "scale8", True, False, True, "rows"), ("last_quad_dropped", 2, 2052, "scale0.5", False, False, True, "rows"),
    ("w_twice", 5, 257, "scale0.5", True, False, False, "dl"), ("w_twice", 3, 1024, "pow2w", True, True, True, "dl"),
    ("w_none", 5, 257, "scale0.5", True, False, False, "dl"), ("w_none", 3, 1024, "pow2w", True, True, True, "dl"),
    ("inv_N", 3, 5, "scale8", False, False, False, "dl"), ("inv_N", 513, 4, "scale30", True, True, True, "dl"),
    ("log_not_log1p", 2, 1000, "confident", False, False, True, "rows"), ("log_not_log1p", 3, 1027, "confident", True, True, False, "rows"),
    ("other_sigmoid", 3, 5, "edges", False, False, False, "dl"), ("other_sigmoid", 2, 1000, "edges", True, False, True, "dl"),
    ("focal_gamma_exp", 3, 5, "scale0.5", False, True, False, "s"), ("focal_gamma_exp", 2, 1000, "scale8", True, True, True, "dl"),
    ("skip_wave", 2, 1000, "scale8", False, False, True, "rows"), ("skip_wave", 3, 1027, "scale0.5", True, False, False, "rows"),
    ("mean_N", 3, 5, "scale8", False, False, False, "loss"), ("mean_N", 257, 3, "scale0.5", True, True, False, "loss")])
def test_mlabel_faults_rejected(fault, N, Cn, kind, weighted, focal, vec, only):
    """each fault on the inputs of tests/test_gpu_multilabel.py::test_bounds; `only`: the output that must show it.  log_not_log1p
    on the confident batch gives rows of exactly 0, which also pass every max-normalised tolerance.  other_sigmoid:
    1 / (1 + expf(-z)) at z = -90 is 1 / inf = 0 where ea / (1 + ea) is 8.2e-40."""
    z, t, w = BM.mlabel_inputs(kind, N, Cn)
    gamma, balance = BM.ML_FOCAL[1]
    for fused in (False, True):
        _ok(_ml_check(z, t, w if weighted else None, focal, gamma, balance, vec, fused))
        _rejected(lambda: _ml_check(z, t, w if weighted else None, focal, gamma, balance, vec, fused, fault, only=(only,)))


def test_mlabel_confident_focal_smallest_b():
    """the confident batch under focal at gamma 1, 2 and 3.5: 1 - exp(-b) cancels, the bracket of the loss and of s widens to
    about 2^-52 / b relative and still admits the emulation; prints the smallest b and the bracket's relative width there"""
    small = (1.0, 0.0)
    for (N, Cn) in ((2, 1000), (3, 1027)):
        z, t, w = BM.mlabel_inputs("confident", N, Cn)
        for gamma, balance in BM.ML_FOCAL:
            got = emu_mlabel(z, t, None, True, gamma, balance, Cn % 4 == 0, False)
            iv = BM.mlabel_intervals(z, t, None, N, Cn, True, gamma, balance, Cn % 4 == 0, rows_dev=got["rows"])
            for k in ("dl", "rows", "loss", "s"):
                _ok(IV.check_interval(got[k], iv[k], "confident focal " + k, None))
            b = float(iv["b"].mid)
            small = min(small, (b, float(iv["s"].half / iv["s"].mid.abs())))
    print("smallest b %.3g, relative half width of s there %.3g" % small)
    assert small[0] < 1e-8


@pytest.mark.parametrize("fault", ["scale_none_beyond", "scale_twice_beyond"])
def test_mlabel_scale_second_trip_faults_rejected(fault):
    """the (1100, 1000) focal batch: the factor s not applied, and applied twice, from element 4096*256 on"""
    N, Cn = BM.ML_BIG
    z, t, w = BM.mlabel_inputs("scale8", N, Cn)
    gamma, balance = BM.ML_FOCAL[1]
    _ok(_ml_check(z, t, w, True, gamma, balance, True, False, only=("dl",)))
    _rejected(lambda: _ml_check(z, t, w, True, gamma, balance, True, False, fault, only=("dl",)))


def emu_dice(I, P, T, deduct, fault=None):
    if I <= 0:
        return torch.tensor(0.0)
    U = P + T - (I if (deduct and fault != "no_deduct") else 0)
    a = F32(2 * I)
    if fault == "2I_exact":
        a = F64(2 * I)
    elif fault in ("2I_trunc24", "2I_trunc23"):                       # the conversion cuts to 24 / 23 significant bits
        k = max((2 * I).bit_length() - int(fault[-2:]), 0)
        a = F32(((2 * I) >> k) << k)
    v = F32(1) + np.log(F32(F64(a) / F64(F32(U))))                    # (the quotient of two fp32 numbers through fp64: one rounding)
    return torch.from_numpy(np.asarray(min(max(v, F32(0)), F32(1)), dtype=F32))


DICE_COUNTS = [(7, 7, 7), (18394, 50000, 50000), (18394, 50000, 50001), (40, 90, 130), (0, 5, 9), (1, 1, 1),
               (4100 * 4100 - 5, 4100 * 4100 - 3, 4100 * 4100 - 2)]


def test_dice_emulation_and_faults():
    """(I, P, T) of the GPU cases.  U not reduced under deduct is rejected wherever the value is not clamped to 1 either way.
    NOT separable and not claimed: (float)(2 I) taken as exact above 2^25 -- the conversion moves 2 I by at most u relative, and
    the bracket allows the division alone one ulp = 2u; no bracket that admits the kernel's own quotient can tell the two.  The
    same holds for a conversion that truncates to 24 bits where the kernel's rounds (at most 2u): both are shown to lie INSIDE
    the bracket, on the GPU case's counts and on 2I = 2^25 + 14 against a U that puts the value at 1e-3, where nothing but the
    quotient and logf round.  The nearest fault that can be told apart is narrowed to: a conversion that keeps 23 bits (up to
    4u; here 6 / 2^25 and 14 / 2^25 of 2I) -- rejected on both."""
    for (I, P, T) in DICE_COUNTS:
        for deduct in (0, 1):
            _ok(IV.check_interval(emu_dice(I, P, T, deduct), BM.dice_interval(I, P, T, deduct), "dice %r" % ((I, P, T, deduct),), None))
    assert float(emu_dice(7, 7, 7, 0)) == 1.0 and float(BM.dice_interval(7, 7, 7, 0).hi) == 1.0
    assert float(BM.dice_interval(7, 7, 7, 1).lo) == 1.0                                         # deduct pushes it above 1: clamped
    assert float(BM.dice_interval(18394, 50000, 50000, 0).lo) > 0.0 and float(BM.dice_interval(18394, 50000, 50001, 0).hi) == 0.0
    for (I, P, T) in ((18394, 50000, 50000), (40, 90, 130)):
        _rejected(lambda: IV.check_interval(emu_dice(I, P, T, 1, "no_deduct"), BM.dice_interval(I, P, T, 1), "dice, U not reduced", None))
    n = 4100 * 4100
    for (I, P, T) in ((n - 5, n - 3, n - 2), (2 ** 24 + 7, 2 ** 24 + 7 + 28782777, 2 ** 24 + 7 + 28782777)):
        assert 2 * I > 2 ** 25 and float(F32(2 * I)) != 2 * I
        iv = BM.dice_interval(I, P, T, 0)
        for fault in ("2I_exact", "2I_trunc24"):
            _ok(IV.check_interval(emu_dice(I, P, T, 0, fault), iv, "dice, %s (not separable)" % fault, None))
        _rejected(lambda: IV.check_interval(emu_dice(I, P, T, 0, "2I_trunc23"), iv, "dice, (float)(2I) cut to 23 bits", None))
