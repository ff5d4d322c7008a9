"""-m gpu: every HIP kernel, called through the C ABI, against fp32 torch-CPU math on the same bf16-rounded
inputs.  Tolerance: outputs are stored as bf16 (half-ulp 2^-9) after fp32 accumulation, so the bound is
max|hip - ref| <= 6e-3 * max|ref| for bf16 tensors and 2e-3 for fp32 reductions (statistics, weight
gradients; limited by bf16 rounding of the staged operands, which the reference reproduces).

On top of that, the conv / depthwise launches are held element by element (resp. channel by channel) to the derived bounds of
tests/bounds_conv.py against fp64 references on the device: check_onload_bound (MFMA launches, operand formed on load and known
as an interval), check_dw_bound (depthwise sweeps, fp32 weights as given), check_sum_bound (weight gradients),
check_stats_bound / check_red_bound (BatchNorm statistics, fused reduce).  Inputs that feed a ReLU mask are moved off the hinge
(bounds_conv.off_hinge).  The sparse-pixel probes at the end put a handful of live pixels at the first / last position and on
both sides of the tile and workgroup boundaries, where the same bounds see one dropped, doubled or misplaced pixel."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from cases import O
from bounds_conv import (act_interval, check_dw_bound, check_onload_bound, check_red_bound, check_stats_bound, dw_dgrad_terms, dw_elem_err,
                         dw_fwd_terms, dw_wgrad_terms, dy_interval, off_hinge, onload_dgrad_terms, onload_elem_err, onload_fwd_terms,
                         wgrad_terms)
from bounds_se import (add_act_interval, bn_bwd_finalize_intervals, bn_fwd_finalize_intervals, bn_fwd_partials, pool_act_terms,
                       stem_dgrad_terms, stem_wgrad_band_rows)
from gpu_util import L, act_in, bf16r, conv_gemm, dy_ref, from_nhwc, grad_in, guarded, nhwc, pack, rand_bn_coefs, relerr
from intervals import U32, Interval, _assert_bound, check_interval, check_store_bound, check_sum_bound, sum_bound
from refs64 import ref_dense_dgrad, ref_dense_wgrad

pytestmark = pytest.mark.gpu
TOL_BF16 = 6e-3
TOL_F32 = 2e-3


def _x(shape, seed):
    return bf16r(O.det_uniform(shape, seed))


DEV = "cuda"            # where the fp64 terms of the per-element bounds are computed


def _nh(t):
    """NCHW (cpu) -> NHWC view"""
    return t.permute(0, 2, 3, 1)


def _xoff(shape, seed, s, t):
    """_x moved off the ReLU hinge of (s, t) (per channel, NCHW)"""
    return off_hinge(_nh(_x(shape, seed)), s, t).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,nparts,count", [(16, 7, 100.0), (48, 64, 3211264.0), (1152, 33, 12544.0),
                                             (24, 1031, 802816.0), (48, 2048, 3211264.0), (1152, 300, 12544.0),    # block-per-channel path
                                             # one partial; both sides of the 64 / 256 threads-per-channel switch; the first
                                             # table with two terms per fp32 accumulator; count = 1 (running_var takes var itself)
                                             (8, 1, 64.0), (24, 256, 50176.0), (24, 257, 50176.0), (16, 1025, 802816.0), (8, 1, 1.0)])
def test_bn_fwd_finalize(C_, nparts, count):
    """C_ channels of the distribution this test always had (mean ~ 0.3 u, var >= 0.5) under the max-normalised 1e-5, plus three
    appended channels (bounds_se.bn_fwd_partials: |mean|/std = 30 and 300, a constant channel whose var takes the clamp); the table
    is built in fp64 and rounded once to fp32, and ALL seven outputs of every channel are held to the brackets of
    bounds_se.bn_fwd_finalize_intervals (fp64 on the fp32 table exactly as given to the kernel)."""
    lib = L.load()
    Ct = C_ + 3
    partial = bn_fwd_partials(O.det_uniform((2, Ct, nparts), 3), count)          # channel-major partial layout
    gamma, beta = 1 + 0.2 * O.det_uniform((Ct,), 4), 0.1 * O.det_uniform((Ct,), 5)
    rm, rv = 0.1 * O.det_uniform((Ct,), 6), 1 + 0.3 * O.det_uniform((Ct,), 7).abs()
    d = lambda t: t.clone().cuda()
    dp, dg, db, drm, drv = d(partial), d(gamma), d(beta), d(rm), d(rv)
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    bn = torch.zeros(8, Ct, device="cuda")
    L.check(lib.mnas_bn_fwd_finalize(dp.data_ptr(), nparts, Ct, count, dg.data_ptr(), db.data_ptr(), drm.data_ptr(),
                                     drv.data_ptr(), nbt.data_ptr(), 0.1, 1e-5, 1, bn.data_ptr(), L.cur_stream()))
    S1, S2 = partial[0].double().sum(-1), partial[1].double().sum(-1)
    mean = S1 / count
    var = (S2 / count - mean * mean).clamp_min(0)
    invstd = 1 / torch.sqrt(var + 1e-5)
    s = gamma.double() * invstd
    t = beta.double() - mean * s
    bn = bn.cpu().double()
    o = slice(0, C_)                                # the ordinary channels, as before
    assert relerr(bn[0][o], s[o]) < 1e-5 and relerr(bn[1][o], t[o]) < 1e-5
    assert relerr(bn[5][o], mean[o]) < 1e-5 and relerr(bn[6][o], invstd[o]) < 1e-5
    assert relerr(drm.cpu()[o], (0.9 * rm.double() + 0.1 * mean)[o]) < 1e-5
    unb = count / (count - 1) if count > 1 else 1.0
    assert relerr(drv.cpu()[o], (0.9 * rv.double() + 0.1 * var * unb)[o]) < 1e-5
    assert int(nbt) == 1
    ivs = bn_fwd_finalize_intervals(partial, count, gamma, beta, rm, rv, 0.1, 1e-5)
    what = "bn_fwd_finalize C %d nparts %d count %g " % (Ct, nparts, count)
    got = {"s": bn[0], "t": bn[1], "mean": bn[5], "invstd": bn[6], "running_mean": drm.cpu(), "running_var": drv.cpu()}
    for k, iv in ivs.items():
        r = check_interval(got[k], iv, what + k, "BatchNorm forward finalize")
        print(what + k, "error / bound %.3f" % r)
    assert float(ivs["invstd"].half[-1]) < 1e-6 * float(ivs["invstd"].mid[-1])     # the constant channel: var < 0, both ends clamped to 0
    # eval mode: coefficients from the running stats, nothing updated
    bn2 = torch.zeros(8, Ct, device="cuda")
    L.check(lib.mnas_bn_fwd_finalize(0, 0, Ct, count, dg.data_ptr(), db.data_ptr(), drm.data_ptr(), drv.data_ptr(),
                                     0, 0.1, 1e-5, 0, bn2.data_ptr(), L.cur_stream()))
    s_e = gamma / torch.sqrt(drv.cpu() + 1e-5)
    assert relerr(bn2[0].cpu()[o], s_e[o]) < 1e-5 and relerr(bn2[1].cpu()[o], (beta - drm.cpu() * s_e)[o]) < 1e-5
    # every channel, the appended ones included: fp32 arithmetic, four roundings (sum, sqrt, division; product; product, difference)
    s64 = gamma.double() / torch.sqrt(drv.cpu().double() + float(torch.tensor(1e-5)))
    t64 = beta.double() - drm.cpu().double() * s64
    _assert_bound(bn2[0].cpu(), s64, 4 * U32 * s64.abs(), what + "eval s", "BatchNorm forward finalize")
    _assert_bound(bn2[1].cpu(), t64, 6 * U32 * (beta.double().abs() + (drm.cpu().double() * s64).abs()), what + "eval t", "BatchNorm forward finalize")


# ---------------------------------------------------------------------------------------------------
PW = [  # N,H,W,Ci,Co
    (2, 12, 12, 16, 48), (2, 12, 12, 48, 16), (3, 9, 7, 72, 24), (2, 6, 7, 96, 576), (2, 5, 5, 1152, 192),
    (5, 16, 16, 32, 16), (2, 7, 7, 240, 40), (1, 28, 28, 40, 240), (2, 14, 14, 576, 96), (1, 9, 9, 480, 80), (3, 5, 5, 120, 40),
    # the widening convs of the <= 28x28 maps: weight-stationary kernel (csrc/mnas_pwx.hip); ragged last pixel group, several
    # groups per workgroup (nparts 13), cout counts that do and do not fill the waves' tiles
    (3, 14, 14, 96, 576), (5, 13, 11, 80, 480), (2, 28, 27, 40, 240), (7, 9, 9, 96, 568), (1, 5, 3, 40, 232), (9, 7, 7, 192, 1152),
    # the DMA-pipelined forward (csrc/mnas_pwf.hip) with a ragged last cout tile (40 of 48) and a ragged last pixel tile (198 pixels):
    # its statistics epilogue stores under the c < Co guard
    (2, 9, 11, 24, 40),
]


@pytest.mark.parametrize("shape", PW)
@pytest.mark.parametrize("virt", [True, False])
def test_pw_fwd(shape, virt):
    """+ check_onload_bound (act-on-load interval; plain x: the zero-width interval) and check_stats_bound (the epilogues sum the
    fp32 accumulator)"""
    N, H, W, Ci, Co = shape
    x = _x((N, Ci, H, W), 1)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 1, 1), 2))
    bias = 0.1 * O.det_uniform((Co,), 3)
    sc, sh = 1 + 0.3 * O.det_uniform((Ci,), 4), 0.2 * O.det_uniform((Ci,), 5)
    a = bf16r(F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))) if virt else x
    ref = F.conv2d(a, w, bias)
    dsc, dsh = sc.cuda(), sh.cuda()
    xd = nhwc(x)
    out, st = conv_gemm(0, N, H, W, Ci, H, W, Co, 1, 1, 0, pack(w, L.PACK_FWD), bias.cuda(),
                        act=act_in(xd, dsc if virt else None, dsh if virt else None), nparts=13, stats=True)
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    iv = act_interval(_nh(x), sc, sh, True, DEV) if virt else Interval.exact(_nh(x), DEV)
    r64, slack, S = onload_fwd_terms(iv, w, bias, device=DEV)
    check_onload_bound(out, r64, slack, S, Ci, "pw_fwd %s virt %d" % (shape, virt), "1x1 forward")
    check_stats_bound(st, r64, onload_elem_err(slack, S, Ci), N * H * W, "pw_fwd %s virt %d" % (shape, virt), "forward statistics")
    st = st.cpu().double().sum(-1)
    assert relerr(st[0], ref.double().sum((0, 2, 3))) < TOL_F32
    assert relerr(st[1], (ref.double() ** 2).sum((0, 2, 3))) < TOL_F32


DENSE = [  # N,H,W,Ci,Co,stride
    (2, 12, 12, 16, 24, 2), (2, 7, 9, 80, 96, 1), (2, 9, 9, 24, 40, 2), (1, 7, 7, 192, 320, 1), (2, 14, 10, 96, 192, 2),
    # N >= 32 with an output plane of <= 256 pixels: the whole-image kernel (csrc/mnas_dimg.hip); ragged planes, cout groups
    (32, 14, 14, 80, 96, 1), (33, 14, 14, 96, 192, 2), (32, 7, 7, 192, 320, 1), (40, 9, 11, 24, 40, 2), (32, 16, 16, 16, 24, 1),
    (35, 13, 15, 40, 80, 2),
    # weight-heavy layer on the 7x7 plane: weight slices register-resident, persistent over images (csrc/mnas_c3r.hip)
    (67, 7, 7, 192, 320, 1), (33, 7, 6, 192, 328, 1), (41, 14, 14, 96, 192, 2), (32, 13, 11, 104, 200, 2),
    # stride 2 on the large maps (>= 100 k output pixels): every wave weight-stationary, gather from global (csrc/mnas_c3x.hip)
    (36, 112, 112, 16, 24, 2), (35, 111, 113, 24, 40, 2), (140, 56, 56, 24, 40, 2),
]


@pytest.mark.parametrize("shape", DENSE)
def test_dense_fwd(shape):
    """+ check_onload_bound and check_stats_bound, as test_pw_fwd"""
    N, H, W, Ci, Co, s = shape
    Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    x = _x((N, Ci, H, W), 1)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 3, 3), 2))
    bias = 0.1 * O.det_uniform((Co,), 3)
    sc, sh = 1 + 0.3 * O.det_uniform((Ci,), 4), 0.2 * O.det_uniform((Ci,), 5)
    a = bf16r(F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)))
    ref = F.conv2d(a, w, bias, stride=s, padding=1)
    dsc, dsh = sc.cuda(), sh.cuda()
    xd = nhwc(x)
    out, st = conv_gemm(0, N, H, W, Ci, Ho, Wo, Co, 3, s, 1, pack(w, L.PACK_FWD), bias.cuda(),
                        act=act_in(xd, dsc, dsh), nparts=5, stats=True)
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    r64, slack, S = onload_fwd_terms(act_interval(_nh(x), sc, sh, True, DEV), w, bias, s, 1, device=DEV)
    check_onload_bound(out, r64, slack, S, 9 * Ci, "dense_fwd %s" % (shape,), "3x3 forward")
    check_stats_bound(st, r64, onload_elem_err(slack, S, 9 * Ci), N * Ho * Wo, "dense_fwd %s" % (shape,), "forward statistics")
    del r64, slack, S
    st = st.cpu().double().sum(-1)
    assert relerr(st[0], ref.double().sum((0, 2, 3))) < TOL_F32
    assert relerr(st[1], (ref.double() ** 2).sum((0, 2, 3))) < TOL_F32


@pytest.mark.parametrize("shape", PW)
@pytest.mark.parametrize("with_resid", [True, False])
def test_pw_dgrad(shape, with_resid):
    """+ check_onload_bound (dy-on-load interval, y off the hinge) and check_red_bound (the reduce sums the gradient as stored)"""
    N, H, W, Ci, Co = shape
    b = rand_bn_coefs(Co, 9, O)
    g, y = _x((N, Co, H, W), 1), _xoff((N, Co, H, W), 2, b[0], b[1])
    dy = dy_ref(g, y, b)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 1, 1), 2))
    ref = F.conv_transpose2d(dy, w)
    resid = _x((N, Ci, H, W), 5)
    if with_resid:
        ref = ref + resid
    gd, yd, bd, rd = nhwc(g), nhwc(y), b.cuda(), nhwc(resid)
    # fused BN-backward reduce for the producer of the conv's input: (sum dz, sum dz*xhat) of (out, y_in, bn_in)
    b_in = rand_bn_coefs(Ci, 22, O)
    y_in = _xoff((N, Ci, H, W), 21, b_in[0], b_in[1])
    yid, bid = nhwc(y_in), b_in.cuda()
    out, st = conv_gemm(1, N, H, W, Co, H, W, Ci, 1, 1, 0, pack(w, L.PACK_DGRAD), None, grad=grad_in(gd, yd, bd),
                        resid=rd if with_resid else None, nparts=11, stats=True, red_y=yid, red_bn=bid)
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    what = "pw_dgrad %s resid %d" % (shape, with_resid)
    r64, slack, S = onload_dgrad_terms(dy_interval(_nh(g), _nh(y), b, True, DEV), w, H, W, 1, 0,
                                       _nh(resid) if with_resid else None, DEV)
    check_onload_bound(out, r64, slack, S, Co, what, "1x1 input gradient")
    check_red_bound(st, out.float(), yid.float(), b_in, N * H * W, what, "fused reduce (GEMM)")
    gq = from_nhwc(out)                                  # the reduce sees g as stored (bf16)
    s_, t_, mu_, is_ = (b_in[i].view(1, -1, 1, 1) for i in (0, 1, 5, 6))
    dz = (gq * ((s_ * y_in + t_) > 0)).double()
    xhat = (y_in * is_ - mu_ * is_).double()
    st = st.cpu().double().sum(-1)
    assert relerr(st[0], dz.sum((0, 2, 3))) < 1e-3
    assert relerr(st[1], (dz * xhat).sum((0, 2, 3))) < 1e-3


@pytest.mark.parametrize("shape", [(2, 14, 14, 576, 96), (1, 20, 20, 72, 24), (4, 28, 28, 240, 40)])
@pytest.mark.parametrize("nparts", [1, 8, 40])
def test_pw_dgrad_plain_dy(shape, nparts):
    """materialised dy (no dy-on-load operand) through the DMA-pipelined 1x1 input gradient, several grid sizes"""
    N, H, W, Ci, Co = shape
    dy = _x((N, Co, H, W), 3)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 1, 1), 2))
    ref = F.conv_transpose2d(dy, w)
    g = L.MnasGradIn()
    dyd = nhwc(dy)
    g.g = dyd.data_ptr()
    out, _ = conv_gemm(1, N, H, W, Co, H, W, Ci, 1, 1, 0, pack(w, L.PACK_DGRAD), None, grad=g, nparts=nparts)
    assert relerr(from_nhwc(out), ref) < TOL_BF16


@pytest.mark.parametrize("shape", DENSE)
def test_dense_dgrad(shape):
    """+ check_onload_bound (dy-on-load interval, y off the hinge)"""
    N, H, W, Ci, Co, s = shape
    Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    b = rand_bn_coefs(Co, 9, O)
    g, y = _x((N, Co, Ho, Wo), 1), _xoff((N, Co, Ho, Wo), 2, b[0], b[1])
    dy = dy_ref(g, y, b)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 3, 3), 2))
    ref = torch.nn.grad.conv2d_input((N, Ci, H, W), w, dy, stride=s, padding=1)
    gd, yd, bd = nhwc(g), nhwc(y), b.cuda()
    out, _ = conv_gemm(1, N, Ho, Wo, Co, H, W, Ci, 3, s, 1, pack(w, L.PACK_DGRAD), None, grad=grad_in(gd, yd, bd), nparts=7)
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    r64, slack, S = onload_dgrad_terms(dy_interval(_nh(g), _nh(y), b, True, DEV), w, H, W, s, 1, None, DEV)
    check_onload_bound(out, r64, slack, S, 9 * Co, "dense_dgrad %s" % (shape,), "3x3 input gradient")


@pytest.mark.parametrize("shape", [(32, 14, 14, 80, 96), (32, 7, 7, 192, 320), (36, 9, 11, 24, 40), (32, 16, 16, 16, 24), (2, 14, 14, 80, 96),
                                   (45, 7, 7, 192, 320), (33, 6, 7, 200, 328)])
@pytest.mark.parametrize("nparts", [5, 32])
def test_dense_dgrad_plain_dy_with_reduce(shape, nparts):
    """stride-1 3x3 input gradient over a MATERIALISED dy (what the engine hands the dense convs), fused BatchNorm-backward
    reduce: whole-image kernel for N >= 32, k_igemm otherwise -- same contract"""
    N, H, W, Ci, Co = shape
    dy = _x((N, Co, H, W), 3)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 3, 3), 2))
    ref = torch.nn.grad.conv2d_input((N, Ci, H, W), w, dy, stride=1, padding=1)
    g = L.MnasGradIn()
    dyd = nhwc(dy)
    g.g = dyd.data_ptr()
    y_in = _x((N, Ci, H, W), 21)
    b_in = rand_bn_coefs(Ci, 22, O)
    yid, bid = nhwc(y_in), b_in.cuda()
    out, st = conv_gemm(1, N, H, W, Co, H, W, Ci, 3, 1, 1, pack(w, L.PACK_DGRAD), None, grad=g, nparts=nparts, stats=True,
                        red_y=yid, red_bn=bid)
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    gq = from_nhwc(out)
    s_, t_, mu_, is_ = (b_in[i].view(1, -1, 1, 1) for i in (0, 1, 5, 6))
    dz = (gq * ((s_ * y_in + t_) > 0)).double()
    xhat = (y_in * is_ - mu_ * is_).double()
    st = st.cpu().double().sum(-1)
    assert relerr(st[0], dz.sum((0, 2, 3))) < 1e-3
    assert relerr(st[1], (dz * xhat).sum((0, 2, 3))) < 1e-3


def _wgrad(N, H, W, Ci, Ho, Wo, Co, k, s, pad, xact, dy, nsplit, accumulate=False, init=None):
    lib = L.load()
    K = k * k * Ci
    partial = torch.full((nsplit, Co, K), float("nan"), device="cuda")
    a = L.MnasConvWgrad()
    a.N, a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.Co = N, H, W, Ci, Ho, Wo, Co
    a.kh = a.kw = k
    a.stride, a.pad, a.nsplit = s, pad, nsplit
    a.x, a.dy, a.partial = xact, dy, partial.data_ptr()
    L.check(lib.mnas_conv_wgrad(C.byref(a), L.cur_stream()), "wgrad")
    grad = init.clone().cuda() if init is not None else torch.full((Co, Ci, k, k), float("nan"), device="cuda")
    L.check(lib.mnas_wgrad_finalize(partial.data_ptr(), nsplit, Co, Ci, k * k, grad.data_ptr(), int(accumulate),
                                    L.cur_stream()))
    return grad.cpu()


@pytest.mark.parametrize("shape", PW)
def test_pw_wgrad(shape):
    """+ check_sum_bound (c = 1) over the act-on-load and dy-on-load intervals, overwrite and accumulate"""
    N, H, W, Ci, Co = shape
    x = _x((N, Ci, H, W), 1)
    sc, sh = 1 + 0.3 * O.det_uniform((Ci,), 4), 0.2 * O.det_uniform((Ci,), 5)
    a = bf16r(F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)))
    b = rand_bn_coefs(Co, 9, O)
    g, y = _x((N, Co, H, W), 6), _xoff((N, Co, H, W), 7, b[0], b[1])
    dy = dy_ref(g, y, b)
    ref = torch.nn.grad.conv2d_weight(a, (Co, Ci, 1, 1), dy)
    xd, gd, yd, bd, dsc, dsh = nhwc(x), nhwc(g), nhwc(y), b.cuda(), sc.cuda(), sh.cuda()
    got = _wgrad(N, H, W, Ci, H, W, Co, 1, 1, 0, act_in(xd, dsc, dsh), grad_in(gd, yd, bd), 3)
    assert relerr(got, ref) < TOL_F32
    r64, S, slack = wgrad_terms(act_interval(_nh(x), sc, sh, True, DEV), dy_interval(_nh(g), _nh(y), b, True, DEV), 1, 1, 0, DEV)
    check_sum_bound(got.to(DEV), r64, S, N * H * W, 3, 1, "pw_wgrad %s" % (shape,), slack, "weight gradient")
    init = O.det_uniform((Co, Ci, 1, 1), 12)
    got2 = _wgrad(N, H, W, Ci, H, W, Co, 1, 1, 0, act_in(xd, dsc, dsh), grad_in(gd, yd, bd), 2, True, init)
    assert relerr(got2, ref + init) < TOL_F32
    i64 = init.double().to(DEV)
    check_sum_bound(got2.to(DEV), r64 + i64, S + i64.abs(), N * H * W, 2, 1, "pw_wgrad %s accumulate" % (shape,), slack, "weight gradient")


@pytest.mark.parametrize("shape", DENSE)
def test_dense_wgrad(shape):
    """+ check_sum_bound (c = 1): plain x, dy-on-load interval"""
    N, H, W, Ci, Co, s = shape
    Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    x = _x((N, Ci, H, W), 1)
    b = rand_bn_coefs(Co, 9, O)
    g, y = _x((N, Co, Ho, Wo), 6), _xoff((N, Co, Ho, Wo), 7, b[0], b[1])
    dy = dy_ref(g, y, b)
    ref = torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, stride=s, padding=1)
    xd, gd, yd, bd = nhwc(x), nhwc(g), nhwc(y), b.cuda()
    got = _wgrad(N, H, W, Ci, Ho, Wo, Co, 3, s, 1, act_in(xd), grad_in(gd, yd, bd), 2)
    assert relerr(got, ref) < TOL_F32
    r64, S, slack = wgrad_terms(Interval.exact(_nh(x), DEV), dy_interval(_nh(g), _nh(y), b, True, DEV), 3, s, 1, DEV)
    check_sum_bound(got.to(DEV), r64, S, N * Ho * Wo, 2, 1, "dense_wgrad %s" % (shape,), slack, "weight gradient")


@pytest.mark.parametrize("shape,nsplit", [((1, 5, 5, 24, 40, 1), 7), ((2, 7, 7, 192, 320, 1), 3), ((1, 6, 6, 16, 24, 2), 5),
                                          ((3, 7, 7, 8, 168, 1), 2)])
def test_dense_wgrad_slabs_and_empty_splits(shape, nsplit):
    """k_wgrad_t: more pixel splits than 64-pixel chunks (empty splits must contribute zeros), slab shapes with padded edge
    tiles in both dimensions, and mnas_conv_wgrad_slabs consistent with a full cover of dW.  + check_sum_bound as test_dense_wgrad."""
    N, H, W, Ci, Co, s = shape
    lib = L.load()
    slabs = lib.mnas_conv_wgrad_slabs(Co, Ci, 9)
    assert 1 <= slabs <= ((Co + 31) // 32) * ((9 * Ci + 31) // 32)
    Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    x = _x((N, Ci, H, W), 31)
    b = rand_bn_coefs(Co, 39, O)
    g, y = _x((N, Co, Ho, Wo), 36), _xoff((N, Co, Ho, Wo), 37, b[0], b[1])
    dy = dy_ref(g, y, b)
    ref = torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, stride=s, padding=1)
    xd, gd, yd, bd = nhwc(x), nhwc(g), nhwc(y), b.cuda()
    got = _wgrad(N, H, W, Ci, Ho, Wo, Co, 3, s, 1, act_in(xd), grad_in(gd, yd, bd), nsplit)
    assert relerr(got, ref) < TOL_F32
    r64, S, slack = wgrad_terms(Interval.exact(_nh(x), DEV), dy_interval(_nh(g), _nh(y), b, True, DEV), 3, s, 1, DEV)
    check_sum_bound(got.to(DEV), r64, S, N * Ho * Wo, nsplit, 1, "dense_wgrad %s nsplit %d" % (shape, nsplit), slack, "weight gradient")
    again = _wgrad(N, H, W, Ci, Ho, Wo, Co, 3, s, 1, act_in(xd), grad_in(gd, yd, bd), nsplit)
    assert torch.equal(got, again)                 # fixed summation order: bit-reproducible


# ---------------------------------------------------------------------------------------------------
DW = [  # N,H,W,C,k
    (2, 12, 12, 48, 3), (2, 12, 12, 72, 5), (2, 7, 9, 240, 5), (3, 14, 14, 480, 3), (5, 7, 7, 1152, 3),
    (2, 33, 20, 32, 3), (2, 28, 28, 72, 5), (3, 7, 7, 576, 5), (1, 40, 24, 120, 5),
    (3, 14, 14, 576, 5), (2, 14, 13, 96, 5),          # the 14-wide planes, on the 4-column strips like every other width
]


@pytest.mark.parametrize("shape", DW)
def test_dw_fwd(shape):
    """+ check_dw_bound (fp32 weights as given) and check_stats_bound (the sweep sums the fp32 accumulator)"""
    lib = L.load()
    N, H, W, C_, k = shape
    x = _x((N, C_, H, W), 1)
    w = O.det_param("t.conv.weight", (C_, 1, k, k), 2)
    bias = 0.1 * O.det_uniform((C_,), 3)
    sc, sh = 1 + 0.3 * O.det_uniform((C_,), 4), 0.2 * O.det_uniform((C_,), 5)
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))      # act-on-read: fp32, not re-rounded to bf16
    ref = F.conv2d(a, w, bias, padding=k // 2, groups=C_)
    xd, dsc, dsh, db = nhwc(x), sc.cuda(), sh.cuda(), bias.cuda()
    wp = pack(w, L.PACK_DW)
    nparts = 40         # >= number of channel blocks (C/64)
    out = torch.empty((N, H, W, C_), dtype=torch.bfloat16, device="cuda")
    rows = lib.mnas_dw_rows(N, H, W, C_, k, nparts, 0)
    assert 1 <= rows <= nparts
    st = torch.full((2, C_, rows), float("nan"), device="cuda")
    a_ = L.MnasDwFwd()
    a_.N, a_.H, a_.W, a_.C, a_.k, a_.nparts = N, H, W, C_, k, nparts
    a_.in_ = act_in(xd, dsc, dsh)
    a_.w, a_.bias, a_.out, a_.stats = wp.data_ptr(), db.data_ptr(), out.data_ptr(), st.data_ptr()
    L.check(lib.mnas_dw_fwd(C.byref(a_), L.cur_stream()), "dw_fwd")
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    r64, S = dw_fwd_terms(act_interval(_nh(x), sc, sh, False, DEV), w.view(C_, k, k), bias, 1, DEV)
    check_dw_bound(out, r64, S, k, "dw_fwd %s" % (shape,), "depthwise forward")
    check_stats_bound(st, r64, dw_elem_err(S, k), N * H * W, "dw_fwd %s" % (shape,), "depthwise statistics")
    st = st.cpu().double().sum(-1)
    assert relerr(st[0], ref.double().sum((0, 2, 3))) < TOL_F32
    assert relerr(st[1], (ref.double() ** 2).sum((0, 2, 3))) < TOL_F32


@pytest.mark.parametrize("shape", DW)
@pytest.mark.parametrize("phase", [0, 12])
def test_dw_bwd(shape, phase):
    """phase 0: fused one-sweep backward; 12: the two-launch form (input gradient, then weight gradient).
    + check_dw_bound (input gradient), check_sum_bound with c = 2 (weight gradient: fp32 x fp32 products), check_red_bound; x (the
    reduce's mask input) and y (dy's) are off the hinge"""
    lib = L.load()
    N, H, W, C_, k = shape
    w = O.det_param("t.conv.weight", (C_, 1, k, k), 2)
    sc, sh = 1 + 0.3 * O.det_uniform((C_,), 4), 0.2 * O.det_uniform((C_,), 5)
    x = _xoff((N, C_, H, W), 1, sc, sh)
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))      # act-on-read / dy-on-read: fp32
    b = rand_bn_coefs(C_, 9, O)
    g, y = _x((N, C_, H, W), 6), _xoff((N, C_, H, W), 7, b[0], b[1])
    dy = dy_ref(g, y, b, rounded=False)
    ref_gin = torch.nn.grad.conv2d_input((N, C_, H, W), w, dy, padding=k // 2, groups=C_)
    ref_dw = torch.nn.grad.conv2d_weight(a, (C_, 1, k, k), dy, padding=k // 2, groups=C_)
    xd, gd, yd, bd, dsc, dsh = nhwc(x), nhwc(g), nhwc(y), b.cuda(), sc.cuda(), sh.cuda()
    wp = pack(w, L.PACK_DW)
    nparts = 37
    gin = torch.empty((N, H, W, C_), dtype=torch.bfloat16, device="cuda")
    rows1 = lib.mnas_dw_rows(N, H, W, C_, k, nparts, 1 if phase == 0 else 3)     # wpartial: fused or weight-gradient-only launch
    # reduce table: written by the fused launch (3-ring geometry) or by the input-gradient-only launch (2 rings)
    rows0 = rows1 if phase == 0 else lib.mnas_dw_rows(N, H, W, C_, k, nparts, 2)
    wpart = torch.full((rows1, k * k, C_), float("nan"), device="cuda")
    a_ = L.MnasDwBwd()
    a_.N, a_.H, a_.W, a_.C, a_.k, a_.nparts = N, H, W, C_, k, nparts
    a_.x, a_.dy = act_in(xd, dsc, dsh), grad_in(gd, yd, bd)
    a_.w, a_.gin, a_.wpartial = wp.data_ptr(), gin.data_ptr(), wpart.data_ptr()
    # fused BN-backward reduce for the producer of x (x is its raw output, b_in its bnbuf)
    b_in = rand_bn_coefs(C_, 22, O)
    b_in[0], b_in[1] = sc, sh                       # rows 0,1 are the same scale/shift the act-on-load uses
    bid = b_in.cuda()
    redp = torch.full((2, C_, rows0), float("nan"), device="cuda")
    a_.red_bn, a_.red_partial = bid.data_ptr(), redp.data_ptr()
    if phase == 0:
        a_.phase = 0
        L.check(lib.mnas_dw_bwd(C.byref(a_), L.cur_stream()), "dw_bwd")
    else:
        for ph in (1, 2):
            a_.phase = ph
            L.check(lib.mnas_dw_bwd(C.byref(a_), L.cur_stream()), "dw_bwd")
    assert relerr(from_nhwc(gin), ref_gin) < TOL_BF16
    what = "dw_bwd %s phase %d" % (shape, phase)
    div = dy_interval(_nh(g), _nh(y), b, False, DEV)
    r64, S = dw_dgrad_terms(div, w.view(C_, k, k), H, W, 1, DEV)
    check_dw_bound(gin, r64, S, k, what, "depthwise input gradient")
    check_red_bound(redp, gin.float(), xd.float(), b_in, N * H * W, what, "fused reduce (depthwise)")
    gq = from_nhwc(gin)
    s_, t_, mu_, is_ = (b_in[i].view(1, -1, 1, 1) for i in (0, 1, 5, 6))
    dz = (gq * ((s_ * x + t_) > 0)).double()
    xhat = (x * is_ - mu_ * is_).double()
    rp = redp.cpu().double().sum(-1)
    assert relerr(rp[0], dz.sum((0, 2, 3))) < 1e-3
    assert relerr(rp[1], (dz * xhat).sum((0, 2, 3))) < 1e-3
    grad = torch.full((C_, 1, k, k), float("nan"), device="cuda")
    L.check(lib.mnas_dw_wgrad_finalize(wpart.data_ptr(), rows1, C_, k, grad.data_ptr(), 0, L.cur_stream()))
    assert relerr(grad.cpu(), ref_dw) < TOL_F32
    r64, S, slack = dw_wgrad_terms(act_interval(_nh(x), sc, sh, False, DEV), div, k, 1, DEV)
    check_sum_bound(grad.view(C_, k, k), r64, S, N * H * W, rows1, 2, what + " dW", slack, "depthwise weight gradient")


# ---------------------------------------------------------------------------------------------------
# stride-2 depthwise (SepConv(reduce=True), mnasnet.py:73-81; csrc/mnas_dw2.hip): forward + statistics, input gradient, weight
# gradient through mnas_dw_fwd / mnas_dw_bwd with stride = 2; odd planes, 5x5, more than 256 channel pairs (two channel blocks)
# + the corners of dw2_plan: C = 8 (4 channel pairs per block, 64 pixel lanes), C = 200 (100 pairs, 2 pixel lanes, 56 idle threads),
# C = 520 (two channel blocks, the second with 4 pairs), 1 x 1 and 2 x 2 planes (Ho = Wo = 1: nparts above the pixel count)
@pytest.mark.parametrize("shape", [(2, 12, 12, 48, 3), (3, 13, 11, 72, 5), (2, 9, 9, 600, 3), (5, 7, 8, 32, 5),
                                   (2, 6, 5, 8, 3), (2, 5, 7, 200, 5), (2, 5, 4, 520, 3), (3, 1, 1, 16, 3), (1, 1, 1, 8, 5),
                                   (2, 2, 2, 24, 5), (2, 2, 2, 8, 3)])
def test_dw_stride2(shape):
    """+ the bounds of test_dw_fwd / test_dw_bwd at stride 2"""
    lib = L.load()
    N, H, W, C_, k = shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // 2 + 1, (W + 2 * p - k) // 2 + 1
    x = _x((N, C_, H, W), 1)
    w = O.det_param("t.conv.weight", (C_, 1, k, k), 2)
    bias = 0.1 * O.det_uniform((C_,), 3)
    sc, sh = 1 + 0.3 * O.det_uniform((C_,), 4), 0.2 * O.det_uniform((C_,), 5)
    a = F.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    ref = F.conv2d(a, w, bias, stride=2, padding=p, groups=C_)
    assert tuple(ref.shape) == (N, C_, Ho, Wo)
    xd, dsc, dsh, db = nhwc(x), sc.cuda(), sh.cuda(), bias.cuda()
    wp = pack(w, L.PACK_DW)
    nparts = 23
    rows = lib.mnas_dw_rows(N, H, W, C_, k, nparts, 4)
    assert 1 <= rows <= nparts
    out = torch.empty((N, Ho, Wo, C_), dtype=torch.bfloat16, device="cuda")
    st = torch.full((2, C_, rows), float("nan"), device="cuda")
    f = L.MnasDwFwd()
    f.N, f.H, f.W, f.C, f.k, f.nparts, f.stride = N, H, W, C_, k, nparts, 2
    f.in_ = act_in(xd, dsc, dsh)
    f.w, f.bias, f.out, f.stats = wp.data_ptr(), db.data_ptr(), out.data_ptr(), st.data_ptr()
    L.check(lib.mnas_dw_fwd(C.byref(f), L.cur_stream()), "dw_fwd stride 2")
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    aiv = act_interval(_nh(x), sc, sh, False, DEV)
    r64, S = dw_fwd_terms(aiv, w.view(C_, k, k), bias, 2, DEV)
    check_dw_bound(out, r64, S, k, "dw_fwd s2 %s" % (shape,), "depthwise forward")
    check_stats_bound(st, r64, dw_elem_err(S, k), N * Ho * Wo, "dw_fwd s2 %s" % (shape,), "depthwise statistics")
    s1, s2 = st[0].cpu().double().sum(-1), st[1].cpu().double().sum(-1)
    assert relerr(s1, ref.double().sum((0, 2, 3))) < 1e-3 and relerr(s2, (ref.double() ** 2).sum((0, 2, 3))) < 1e-3
    # backward: dy-on-read from (g, y, coef) at the OUTPUT resolution
    b = rand_bn_coefs(C_, 9, O)
    g, y = _x((N, C_, Ho, Wo), 6), _xoff((N, C_, Ho, Wo), 7, b[0], b[1])
    dy = dy_ref(g, y, b, rounded=False)
    ref_gin = torch.nn.grad.conv2d_input((N, C_, H, W), w, dy, stride=2, padding=p, groups=C_)
    ref_dw = torch.nn.grad.conv2d_weight(a, (C_, 1, k, k), dy, stride=2, padding=p, groups=C_)
    gd, yd, bd = nhwc(g), nhwc(y), b.cuda()
    gin = torch.empty((N, H, W, C_), dtype=torch.bfloat16, device="cuda")
    wrows = lib.mnas_dw_rows(N, H, W, C_, k, nparts, 7)
    wpart = torch.full((wrows, k * k, C_), float("nan"), device="cuda")
    d = L.MnasDwBwd()
    d.N, d.H, d.W, d.C, d.k, d.nparts, d.stride = N, H, W, C_, k, nparts, 2
    d.x, d.dy = act_in(xd, dsc, dsh), grad_in(gd, yd, bd)
    d.w, d.gin, d.wpartial = wp.data_ptr(), gin.data_ptr(), wpart.data_ptr()
    for ph in (1, 2):
        d.phase = ph
        L.check(lib.mnas_dw_bwd(C.byref(d), L.cur_stream()), "dw_bwd stride 2")
    assert relerr(from_nhwc(gin), ref_gin) < TOL_BF16
    div = dy_interval(_nh(g), _nh(y), b, False, DEV)
    r64, S = dw_dgrad_terms(div, w.view(C_, k, k), H, W, 2, DEV)
    check_dw_bound(gin, r64, S, k, "dw_bwd s2 %s" % (shape,), "depthwise input gradient")
    grad = torch.full((C_, 1, k, k), float("nan"), device="cuda")
    L.check(lib.mnas_dw_wgrad_finalize(wpart.data_ptr(), wrows, C_, k, grad.data_ptr(), 0, L.cur_stream()))
    assert relerr(grad.cpu(), ref_dw) < TOL_F32
    r64, S, slack = dw_wgrad_terms(aiv, div, k, 2, DEV)
    check_sum_bound(grad.view(C_, k, k), r64, S, N * Ho * Wo, wrows, 2, "dw_bwd s2 %s dW" % (shape,), slack, "depthwise weight gradient")
    d.phase = 0                                        # the fused one-sweep form exists for stride 1 only
    assert lib.mnas_dw_bwd(C.byref(d), L.cur_stream()) == L.EINVAL


# ---------------------------------------------------------------------------------------------------
# (N, H, W[, Co]): W % 4 == 0 with 32 couts runs the band kernels (csrc/mnas_stem.hip; weight gradient also needs Wo % 8 == 0),
# everything else the im2col staging of k_igemm / k_wgrad; partial last bands, odd heights, more bands than workgroups
@pytest.mark.parametrize("shape", [(2, 12, 12), (3, 33, 21), (1, 64, 64), (3, 40, 48), (2, 37, 32), (11, 18, 16), (2, 224, 224),
                                   (2, 24, 24, 16), (1, 34, 80),
                                   # the smallest band shape (one output row); odd H with a partial last band for the forward's
                                   # 8-row and the weight gradient's 4-row bands
                                   (1, 2, 16), (3, 33, 48)])
def test_stem(shape):
    """+ check_sum_bound (c = 1) on the weight gradient after mnas_wgrad_finalize -- the image operand is exact (the kernels round
    it to bf16, the reference takes bf16r(x)), dy the bf16 dy-on-load interval with y off the hinge -- and stem_dgrad_terms on the
    input gradient, whose weights are handed over in fp32, NOT bf16-representable (the kernel's own rounding is under test)."""
    lib = L.load()
    N, H, W = shape[:3]
    Co = shape[3] if len(shape) > 3 else 32
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = O.det_uniform((N, 3, H, W), 1)
    w_raw = O.det_param("t.conv.weight", (Co, 3, 3, 3), 2)
    w = bf16r(w_raw)
    assert not torch.equal(w, w_raw)
    bias = 0.1 * O.det_uniform((Co,), 3)
    ref = F.conv2d(bf16r(x), w, bias, stride=2, padding=1)
    xd = x.cuda()
    wp = pack(w.view(Co, 27, 1, 1), L.PACK_FWD)
    nparts = 9
    out, out_chk = guarded((N, Ho, Wo, Co), torch.bfloat16)
    st, st_chk = guarded((2, Co, nparts), torch.float32)
    a = L.MnasStemFwd()
    a.N, a.H, a.W, a.Ho, a.Wo, a.Co, a.nparts = N, H, W, Ho, Wo, Co, nparts
    db = bias.cuda()
    a.x, a.w, a.bias, a.out, a.stats = xd.data_ptr(), wp.data_ptr(), db.data_ptr(), out.data_ptr(), st.data_ptr()
    L.check(lib.mnas_stem_fwd(C.byref(a), L.cur_stream()), "stem_fwd")
    out_chk("stem_fwd out")
    st_chk("stem_fwd stats")
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    st = st.cpu().double().sum(-1)
    assert relerr(st[0], ref.double().sum((0, 2, 3))) < TOL_F32
    assert relerr(st[1], (ref.double() ** 2).sum((0, 2, 3))) < TOL_F32
    # wgrad
    b = rand_bn_coefs(Co, 9, O)
    g, y = _x((N, Co, Ho, Wo), 6), _xoff((N, Co, Ho, Wo), 7, b[0], b[1])
    dy = dy_ref(g, y, b)
    ref_dw = torch.nn.grad.conv2d_weight(bf16r(x), (Co, 3, 3, 3), dy, stride=2, padding=1)
    gd, yd, bd = nhwc(g), nhwc(y), b.cuda()
    partial, partial_chk = guarded((nparts, Co, 27), torch.float32)
    s = L.MnasStemWgrad()
    s.N, s.H, s.W, s.Ho, s.Wo, s.Co, s.nparts = N, H, W, Ho, Wo, Co, nparts
    s.x, s.dy, s.partial = xd.data_ptr(), grad_in(gd, yd, bd), partial.data_ptr()
    L.check(lib.mnas_stem_wgrad(C.byref(s), L.cur_stream()), "stem_wgrad")
    partial_chk("stem_wgrad partial")
    grad, grad_chk = guarded((Co, 3, 3, 3), torch.float32)
    L.check(lib.mnas_wgrad_finalize(partial.data_ptr(), nparts, Co, 27, 1, grad.data_ptr(), 0, L.cur_stream()))
    grad_chk("stem dW")
    assert relerr(grad.cpu(), ref_dw) < TOL_F32
    div = dy_interval(_nh(g), _nh(y), b, True, DEV)
    r64, S, slack = wgrad_terms(Interval.exact(_nh(bf16r(x)), DEV), div, 3, 2, 1, DEV)
    r = check_sum_bound(grad, r64, S, N * Ho * Wo, nparts, 1, "stem_wgrad %s" % (shape,), slack, "stem weight gradient")
    print("stem_wgrad %s error / bound %.3f" % (shape, r))
    del r64, S, slack
    # input gradient (dL/d image, fp32 NCHW): bf16 dy and weights, fp32 accumulate; with the fused input normalisation's scale
    ref_dx = torch.nn.grad.conv2d_input((N, 3, H, W), w, bf16r(dy), stride=2, padding=1)
    w32 = w_raw.cuda().contiguous()                # fp32 master weights: the kernel rounds them to bf16 itself
    for aff in (None, torch.tensor([[2.0, 0.5, 1.25], [0.1, 0.2, 0.3]])):
        dx, dx_chk = guarded((N, 3, H, W), torch.float32)
        affd = aff.cuda().contiguous() if aff is not None else None
        gi = grad_in(gd, yd, bd)
        L.check(lib.mnas_stem_dgrad(C.byref(gi), w32.data_ptr(), N, H, W, Ho, Wo, Co, affd.data_ptr() if aff is not None else None,
                                    dx.data_ptr(), L.cur_stream()), "stem_dgrad")
        dx_chk("stem_dgrad dx")
        want = ref_dx if aff is None else ref_dx * aff[0].view(1, 3, 1, 1)
        assert relerr(dx.cpu(), want) < TOL_F32
        r64, bound = stem_dgrad_terms(div, w, H, W, aff, DEV)
        r = _assert_bound(dx, r64, bound, "stem_dgrad %s affine %d" % (shape, aff is not None), "stem input gradient")
        print("stem_dgrad %s error / bound %.3f" % (shape, r))
    assert lib.mnas_stem_dgrad(C.byref(gi), w32.data_ptr(), N, H, W, Ho + 1, Wo, Co, None, dx.data_ptr(), L.cur_stream()) == L.EINVAL


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,rows", [(16, 1000), (48, 777), (72, 301), (1152, 98), (240, 1570)])
def test_bn_bwd(C_, rows):
    lib = L.load()
    g, y = _x((rows, C_), 1), _x((rows, C_), 2)
    b = rand_bn_coefs(C_, 9, O)
    gd, yd, bd = g.to(torch.bfloat16).cuda(), y.to(torch.bfloat16).cuda(), b.clone().cuda()
    nparts = 7
    partial = torch.full((2, C_, nparts), float("nan"), device="cuda")
    L.check(lib.mnas_bn_bwd_reduce(gd.data_ptr(), yd.data_ptr(), bd.data_ptr(), rows, C_, nparts, partial.data_ptr(),
                                   L.cur_stream()))
    s, t, mean, invstd = b[0], b[1], b[5], b[6]
    dz = (g * ((s * y + t) > 0)).double()
    xhat = ((y - mean) * invstd).double()
    S1, S2 = dz.sum(0), (dz * xhat).sum(0)
    p = partial.cpu().double().sum(-1)
    assert relerr(p[0], S1) < 1e-4 and relerr(p[1], S2) < 1e-4
    dgamma = torch.full((C_,), 2.0, device="cuda")
    dbeta = torch.full((C_,), 3.0, device="cuda")
    L.check(lib.mnas_bn_bwd_finalize(partial.data_ptr(), nparts, C_, float(rows), bd.data_ptr(), dgamma.data_ptr(),
                                     dbeta.data_ptr(), 1, L.cur_stream()))
    assert relerr(dgamma.cpu() - 2.0, S2) < 1e-4 and relerr(dbeta.cpu() - 3.0, S1) < 1e-4
    # the finalize alone: fp64 on the fp32 table the reduce wrote, brackets of bounds_se.bn_bwd_finalize_intervals
    ivs = bn_bwd_finalize_intervals(partial.cpu(), float(rows), b, torch.full((C_,), 2.0), torch.full((C_,), 3.0))
    fin = {"c1": bd[2], "c2": bd[3], "c3": bd[4], "dgamma": dgamma, "dbeta": dbeta}
    for k, iv in ivs.items():
        check_interval(fin[k].cpu(), iv, "bn_bwd_finalize C %d rows %d %s" % (C_, rows, k), "BatchNorm backward finalize")
    out = bd.cpu().double()
    sd = s.double()
    assert relerr(out[2], sd) < 1e-6
    assert relerr(out[3], -sd * invstd.double() * S2 / rows) < 1e-4
    assert relerr(out[4], sd * (mean.double() * invstd.double() * S2 / rows - S1 / rows)) < 1e-4
    # the coefficients reproduce native_batch_norm_backward's dy
    dy_formula = sd * invstd.double() / sd * 0 + (sd * (dz - S1 / rows - xhat * S2 / rows))
    dy_coef = out[2] * dz + out[3] * y.double() + out[4]
    assert relerr(dy_coef, dy_formula) < 1e-4


@pytest.mark.parametrize("C_,rows,HW", [(16, 500, 50), (320, 98, 49), (96, 392, 196)])
def test_add_act_and_layouts(C_, rows, HW):
    lib = L.load()
    a, b = _x((rows, C_), 1), _x((rows, C_), 2)
    sa, ta = 1 + 0.3 * O.det_uniform((C_,), 4), 0.2 * O.det_uniform((C_,), 5)
    sb, tb = 1 + 0.3 * O.det_uniform((C_,), 6), 0.2 * O.det_uniform((C_,), 7)
    ad, bd = a.to(torch.bfloat16).cuda(), b.to(torch.bfloat16).cuda()
    dsa, dta, dsb, dtb = sa.cuda(), ta.cuda(), sb.cuda(), tb.cuda()
    ref = F.relu(a * sa + ta) + F.relu(b * sb + tb)
    out = torch.empty((rows, C_), dtype=torch.bfloat16, device="cuda")
    N = rows // HW
    onchw = torch.full((N, C_, HW), float("nan"), device="cuda")
    A, B = act_in(ad, dsa, dta), act_in(bd, dsb, dtb)
    L.check(lib.mnas_add_act(C.byref(A), C.byref(B), rows, C_, out.data_ptr(), onchw.data_ptr(), HW, L.cur_stream()))
    assert relerr(out.float().cpu(), ref) < TOL_BF16
    assert relerr(onchw.cpu(), ref.view(N, HW, C_).permute(0, 2, 1)) < 1e-6
    # per element: the fp32 NCHW output inside the bracket of relu(fma) + relu(fma) and one add; the bf16 output one rounding of it
    iv = add_act_interval(act_interval(a, sa, ta, False, DEV), act_interval(b, sb, tb, False, DEV))
    check_store_bound(out, iv, "add_act C %d bf16" % C_, "add_act")
    check_interval(onchw.permute(0, 2, 1).reshape(rows, C_), iv, "add_act C %d fp32 NCHW" % C_, "add_act")
    # identity + single input
    A2 = act_in(ad)
    L.check(lib.mnas_add_act(C.byref(A2), None, rows, C_, out.data_ptr(), 0, HW, L.cur_stream()))
    assert relerr(out.float().cpu(), a) == 0.0
    # incoming gradient conversion
    src = O.det_uniform((N, C_, HW), 8)
    dst = torch.empty((N, HW, C_), dtype=torch.bfloat16, device="cuda")
    sd = src.cuda()
    L.check(lib.mnas_nchw_f32_to_nhwc_bf16(sd.data_ptr(), dst.data_ptr(), N, C_, HW, L.cur_stream()))
    assert relerr(dst.float().cpu(), bf16r(src).permute(0, 2, 1)) == 0.0


def test_adam_matches_torch():
    lib = L.load()
    n = 10007
    p0, g0 = O.det_uniform((n,), 1), O.det_uniform((n,), 2)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=1e-3)
    pd, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in range(1, 4):
        g = g0 * step
        p.grad = g.clone()
        opt.step()
        gd = g.cuda()
        L.check(lib.mnas_adam_step(pd.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8,
                                   0.0, step, 1.0, L.cur_stream()))
    assert relerr(pd.cpu(), p.detach()) < 1e-5


def _opt_state(n):
    import bounds_tail as BT
    p, g, m, v, buf = BT.opt_data(n, seed=n)
    return dict(p=p, g=g, m=m, v=v, buf=buf)


@pytest.mark.parametrize("n", [1, 255, 257, 10007, 2048 * 256 + 300])
def test_optimizer_per_element_bracket(n):
    """ONE launch of mnas_adam_step / mnas_rmsprop_step / mnas_sgd_step from a given non-zero state (bounds_tail.opt_case): every
    element of every output inside the bracket propagated through the kernel's own roundings, with per-element scales 2^-20 .. 2^4
    in p and g, exact zeros, elements with v = 0 and g = 0 (denom = eps) and with a tiny v; the runs start at element offsets 0, 1
    and 3 of guarded buffers.  The last size exceeds opt_blocks' grid of 2048 workgroups of 256, so a lane takes the grid-stride
    loop's second trip.  Adam: step 1 / 2 / 1000 / 100000, weight decay, grad_scale 1, 1/8, 1/3; RMSprop with and without momentum;
    SGD with momentum, dampening, Nesterov, first and second step."""
    import bounds_tail as BT
    import intervals as IV
    assert BT.OPT_SIZES[-1] > BT.OPT_GRID_CAP == 2048 * 256 and n in BT.OPT_SIZES
    st = _opt_state(n)
    worst, k = 0.0, 0
    for step in (1, 2, 1000, 100000):
        for wd in (0.0, 1e-2):
            for gs in (1.0, 0.125, 1.0 / 3):
                a = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=wd, step=step, gscale=gs)
                worst, k = max(worst, BT.opt_case("adam", st, a, (0, 1, 3)[k % 3])), k + 1
    for mom in (0.0, 0.9):
        for wd in (0.0, 1e-2):
            a = dict(lr=1e-2, alpha=0.99, eps=1e-8, wd=wd, momentum=mom, gscale=1.0 / 3)
            worst, k = max(worst, BT.opt_case("rmsprop", st, a, (0, 1, 3)[k % 3])), k + 1
        for damp in (0.0, 0.5):
            for nest in (0, 1):
                for step in (1, 2):
                    a = dict(lr=1e-2, momentum=mom, dampening=damp, wd=1e-2 * nest, nesterov=nest, step=step, gscale=0.125)
                    worst, k = max(worst, BT.opt_case("sgd", st, a, (0, 1, 3)[k % 3])), k + 1
    print("optimizers n %d: %d launches, worst error / bracket %.4f" % (n, k, worst), {"optimizers": IV.WORST.get("optimizers")})
    assert worst <= 1.0


def test_run_ops_batch():
    """The batched launcher reproduces the individual calls (pack -> pw fwd -> bn finalize)."""
    lib = L.load()
    N, H, W, Ci, Co = 2, 12, 12, 16, 48
    x = _x((N, Ci, H, W), 1)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 1, 1), 2))
    xd, wd = nhwc(x), w.cuda().contiguous()
    wp = torch.empty(lib.mnas_packed_bytes(L.PACK_FWD, Co, Ci, 1, 1), dtype=torch.uint8, device="cuda")
    out = torch.empty((N, H, W, Co), dtype=torch.bfloat16, device="cuda")
    nparts = 4
    st = torch.empty((2, Co, nparts), device="cuda")
    gamma, beta = torch.ones(Co, device="cuda"), torch.zeros(Co, device="cuda")
    rm, rv = torch.zeros(Co, device="cuda"), torch.ones(Co, device="cuda")
    bn = torch.zeros(8, Co, device="cuda")
    ops = (L.MnasOp * 3)()
    L.set_op(ops[0], L.OP_PACK_WEIGHTS, kind=L.PACK_FWD, Co=Co, Ci=Ci, kh=1, kw=1, w=wd, dst=wp)
    L.set_op(ops[1], L.OP_CONV_GEMM, mode=0, N=N, Hi=H, Wi=W, Ci=Ci, Ho=H, Wo=W, Co=Co, kh=1, kw=1, stride=1, pad=0, nparts=nparts,
             act=(xd, None, None), w=wp, out=out, stats=st)
    L.set_op(ops[2], L.OP_BN_FWD_FINALIZE, nparts=nparts, C=Co, training=1, count=float(N * H * W), momentum=0.1, eps=1e-5,
             partial=st, gamma=gamma, beta=beta, rmean=rm, rvar=rv, nbt=None, bnbuf=bn)
    failed = C.c_int(-1)
    L.check(lib.mnas_run_ops(ops, 3, L.cur_stream(), C.byref(failed)), "run_ops")
    ref = F.conv2d(x, w)
    assert relerr(from_nhwc(out), ref) < TOL_BF16
    mean = ref.double().mean((0, 2, 3))
    assert relerr(bn[5].cpu(), mean) < TOL_F32
    # a bad opcode is reported, not ignored
    ops[1].opcode = 999
    assert lib.mnas_run_ops(ops, 3, L.cur_stream(), C.byref(failed)) != 0 and failed.value == 1


@pytest.mark.parametrize("C_,nparts", [(16, 1024), (40, 257), (1152, 64), (1152, 513), (8, 1), (24, 256), (16, 1025)])
def test_bn_bwd_finalize_long_rows(C_, nparts):
    """Both finalize shapes (wave per channel / block per channel) against an fp64 sum of the same partial table; + the brackets of
    bounds_se.bn_bwd_finalize_intervals on rows 2..4, dgamma and dbeta (1025 partials: two terms per fp32 accumulator)."""
    lib = L.load()
    partial = O.det_uniform((2, C_, nparts), 31)
    b = rand_bn_coefs(C_, 9, O)
    bd, pd = b.clone().cuda(), partial.clone().cuda()
    dgamma, dbeta = torch.zeros(C_, device="cuda"), torch.zeros(C_, device="cuda")
    rows = 12345.0
    L.check(lib.mnas_bn_bwd_finalize(pd.data_ptr(), nparts, C_, rows, bd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                     0, L.cur_stream()))
    S = partial.double().sum(-1)
    s, mean, invstd = b[0].double(), b[5].double(), b[6].double()
    out = bd.cpu().double()
    assert relerr(dbeta.cpu(), S[0]) < 1e-5 and relerr(dgamma.cpu(), S[1]) < 1e-5
    assert relerr(out[3], -s * invstd * S[1] / rows) < 1e-5
    assert relerr(out[4], s * (mean * invstd * S[1] / rows - S[0] / rows)) < 1e-5
    ivs = bn_bwd_finalize_intervals(partial, rows, b)
    fin = {"c1": bd[2], "c2": bd[3], "c3": bd[4], "dgamma": dgamma, "dbeta": dbeta}
    for k, iv in ivs.items():
        r = check_interval(fin[k].cpu(), iv, "bn_bwd_finalize C %d nparts %d %s" % (C_, nparts, k), "BatchNorm backward finalize")
        print("bn_bwd_finalize C %d nparts %d %s error / bound %.3f" % (C_, nparts, k, r))


@pytest.mark.parametrize("nsplit,Co,Ci,taps,acc", [(5, 24, 16, 1, 0), (300, 16, 48, 1, 1), (300, 16, 48, 1, 0),
                                                   (1024, 16, 32, 1, 1), (129, 8, 8, 9, 1)])
def test_wgrad_finalize_split_ranges(nsplit, Co, Ci, taps, acc):
    """Split ranges longer than one block's share are cut over grid.y (atomic combine) in accumulate mode and walked by
    one block in overwrite mode; dense [Co][taps*Ci] -> [Co][Ci][taps] and depthwise [taps][C] -> [C][taps] relayouts."""
    lib = L.load()
    part = O.det_uniform((nsplit, Co, taps * Ci), 41)
    init = O.det_uniform((Co, Ci, taps), 42)
    grad = init.clone().cuda()
    L.check(lib.mnas_wgrad_finalize(part.cuda().data_ptr(), nsplit, Co, Ci, taps, grad.data_ptr(), acc, L.cur_stream()))
    ref = part.double().sum(0).view(Co, taps, Ci).permute(0, 2, 1) + (init.double() if acc else 0)
    assert relerr(grad.cpu(), ref) < 1e-5
    # check_sum_bound: M = nsplit terms in some fixed tree (nsplit - 1 adds however it is cut), the accumulate target is the +1; c = 1
    lay = lambda t: t.double().abs().sum(0).view(Co, taps, Ci).permute(0, 2, 1)
    r = check_sum_bound(grad.cpu(), ref, lay(part) + (init.double().abs() if acc else 0), nsplit, 0, 1,
                        "wgrad_finalize nsplit %d acc %d" % (nsplit, acc), None, "weight-gradient finalize")
    k = 3
    dpart = O.det_uniform((nsplit, k * k, Co), 43)
    dinit = O.det_uniform((Co, k * k), 44)
    dgrad = dinit.clone().cuda()
    L.check(lib.mnas_dw_wgrad_finalize(dpart.cuda().data_ptr(), nsplit, Co, k, dgrad.data_ptr(), acc, L.cur_stream()))
    dref = dpart.double().sum(0).t() + (dinit.double() if acc else 0)
    assert relerr(dgrad.cpu(), dref) < 1e-5
    r2 = check_sum_bound(dgrad.cpu(), dref, dpart.double().abs().sum(0).t() + (dinit.double().abs() if acc else 0), nsplit, 0, 1,
                         "dw_wgrad_finalize nsplit %d acc %d" % (nsplit, acc), None, "weight-gradient finalize")
    print("wgrad finalizes nsplit %d acc %d: error / bound %.3f, %.3f" % (nsplit, acc, r, r2))


# ---------------------------------------------------------------------------------------------------
# fused 1x1 backward (input gradient + weight gradient + BatchNorm-backward reduce of x's producer)
PWB = [  # N,H,W,Ci,Co  -- every supported (cin tiles, cout tiles) pair; ragged pixel counts (tile tails)
    (2, 12, 12, 32, 16), (3, 11, 9, 48, 16), (2, 13, 12, 16, 48), (2, 9, 9, 24, 72), (2, 10, 9, 72, 24),
    (1, 9, 8, 40, 240), (1, 11, 7, 240, 40), (1, 9, 7, 480, 80), (1, 10, 7, 576, 96), (2, 9, 8, 40, 120), (2, 11, 7, 120, 40),
]


@pytest.mark.parametrize("shape", PWB)
@pytest.mark.parametrize("variant", ["virt_red", "plain_resid", "virt"])
@pytest.mark.parametrize("nparts", [1, 3])
def test_pw_bwd_fused(shape, variant, nparts):
    """+ check_onload_bound (gin), check_sum_bound c = 1 (dW over both intervals), check_red_bound; x and y off the hinge"""
    lib = L.load()
    N, H, W, Ci, Co = shape
    assert lib.mnas_pw_bwd_supported(Ci, Co) == 1
    M = N * H * W
    virt = variant != "plain_resid"
    bx = rand_bn_coefs(Ci, 22, O)                         # bnbuf of x's producer: rows 0/1 = scale/shift
    x = _xoff((N, Ci, H, W), 1, bx[0], bx[1])
    a = bf16r(F.relu(x * bx[0].view(1, -1, 1, 1) + bx[1].view(1, -1, 1, 1))) if virt else x
    b = rand_bn_coefs(Co, 9, O)
    g, y = _x((N, Co, H, W), 6), _xoff((N, Co, H, W), 7, b[0], b[1])
    dy = dy_ref(g, y, b)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 1, 1), 2))
    resid = _x((N, Ci, H, W), 5)
    ref_gin = F.conv_transpose2d(dy, w) + (resid if variant == "plain_resid" else 0)
    ref_dw = torch.nn.grad.conv2d_weight(a, (Co, Ci, 1, 1), dy)
    xd, gd, yd, bd, bxd, rd = nhwc(x), nhwc(g), nhwc(y), b.cuda(), bx.cuda(), nhwc(resid)
    gin = torch.full((N, H, W, Ci), float("nan"), dtype=torch.bfloat16, device="cuda")
    wpart = torch.full((nparts, Co, Ci), float("nan"), device="cuda")
    redp = torch.full((2, Ci, nparts), float("nan"), device="cuda")
    c = L.MnasPwBwd()
    c.M, c.Ci, c.Co, c.nparts = M, Ci, Co, nparts
    c.x = act_in(xd, bxd[0], bxd[1]) if virt else act_in(xd)
    c.dy = grad_in(gd, yd, bd)
    c.w, c.gin, c.wpartial = L.ptr(pack(w, L.PACK_DGRAD)), L.ptr(gin), L.ptr(wpart)
    c.resid = L.ptr(rd) if variant == "plain_resid" else None
    if variant == "virt_red":
        c.red_partial, c.red_y, c.red_bn = L.ptr(redp), L.ptr(xd), L.ptr(bxd)
    L.check(lib.mnas_pw_bwd(C.byref(c), L.cur_stream()), "pw_bwd")
    assert relerr(from_nhwc(gin), ref_gin) < TOL_BF16
    grad = torch.full((Co, Ci, 1, 1), float("nan"), device="cuda")
    L.check(lib.mnas_wgrad_finalize(wpart.data_ptr(), nparts, Co, Ci, 1, grad.data_ptr(), 0, L.cur_stream()))
    assert relerr(grad.cpu(), ref_dw) < TOL_F32
    what = "pw_bwd %s %s nparts %d" % (shape, variant, nparts)
    div = dy_interval(_nh(g), _nh(y), b, True, DEV)
    r64, slack, S = onload_dgrad_terms(div, w, H, W, 1, 0, _nh(resid) if variant == "plain_resid" else None, DEV)
    check_onload_bound(gin, r64, slack, S, Co, what + " gin", "fused 1x1 backward: gin")
    aiv = act_interval(_nh(x), bx[0], bx[1], True, DEV) if virt else Interval.exact(_nh(x), DEV)
    r64, S, slack = wgrad_terms(aiv, div, 1, 1, 0, DEV)
    check_sum_bound(grad, r64, S, M, nparts, 1, what + " dW", slack, "fused 1x1 backward: dW")
    if variant == "virt_red":
        check_red_bound(redp, gin.float(), xd.float(), bx, M, what, "fused 1x1 backward: reduce")
        gq = from_nhwc(gin)                               # the reduce sees g as stored (bf16)
        s_, t_, mu_, is_ = (bx[i].view(1, -1, 1, 1) for i in (0, 1, 5, 6))
        dz = (gq * ((s_ * x + t_) > 0)).double()
        xhat = (x * is_ - mu_ * is_).double()
        st = redp.cpu().double().sum(-1)
        assert relerr(st[0], dz.sum((0, 2, 3))) < 1e-3
        assert relerr(st[1], (dz * xhat).sum((0, 2, 3))) < 1e-3


def test_pw_bwd_rejects_unsupported():
    lib = L.load()
    assert lib.mnas_pw_bwd_supported(96, 576) == 0 and lib.mnas_pw_bwd_supported(12, 16) == 0
    assert lib.mnas_pw_bwd_supported(576, 96) == 1 and lib.mnas_pw_bwd_supported(480, 80) == 1
    c = L.MnasPwBwd()
    c.M, c.Ci, c.Co, c.nparts = 64, 96, 576, 4
    assert lib.mnas_pw_bwd(C.byref(c), L.cur_stream()) == 10001          # MNAS_EINVAL


def test_pack_weights_batch_matches_single():
    """One batched launch packs what the per-tensor entry point packs (all three kinds, ragged shapes)."""
    lib = L.load()
    cases = [(L.PACK_FWD, 24, 16, 9), (L.PACK_DGRAD, 24, 16, 9), (L.PACK_FWD, 40, 240, 1), (L.PACK_DGRAD, 40, 240, 1),
             (L.PACK_DW, 72, 1, 25), (L.PACK_FWD, 32, 27, 1)]
    ws, singles, batched = [], [], []
    host = (L.MnasPackDesc * len(cases))()
    for n, (kind, Co, Ci, taps) in enumerate(cases):
        k = int(round(taps ** 0.5))
        shape = (Co, Ci, k, k) if k * k == taps else (Co, Ci, 1, taps)
        w = O.det_uniform(shape, 50 + n).cuda().contiguous()
        nbytes = lib.mnas_packed_bytes(kind, Co, Ci, 1, taps)
        a = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        b = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
        L.check(lib.mnas_pack_weights(w.data_ptr(), kind, Co, Ci, 1, taps, a.data_ptr(), L.cur_stream()))
        host[n].w, host[n].dst, host[n].kind, host[n].Co, host[n].Ci, host[n].taps = w.data_ptr(), b.data_ptr(), kind, Co, Ci, taps
        ws.append(w); singles.append(a); batched.append(b)
    dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    L.check(lib.mnas_pack_weights_batch(dev.data_ptr(), len(cases), L.cur_stream()))
    torch.cuda.synchronize()
    for a, b in zip(singles, batched):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------
# Sparse-pixel probes.  A worst-case bound over M pixels grows with M, so one pixel dropped from (doubled in, misplaced in) a long
# sum of dense operands can hide inside it.  Here all but a handful of pixels contribute exactly zero -- the live ones sit at the
# first and last position, on both sides of the first tile boundary and of a workgroup boundary, and at the image corners for
# k > 1 -- and the operands need no transform (plain x, materialised dy; where the ABI takes a dy-on-load operand only, the
# identity coefficients below, under which fma(c1, g, fma(c2, y, c3)) = g exactly).  S then holds only those terms and the same
# check_sum_bound is a few 1e-5 of ONE product.
def _ident_bn(C_):
    """bnbuf rows under which s*y+t = y, dy = g and xhat = y exactly: (s,t,c1,c2,c3,mean,invstd) = (1,0,1,0,0,0,1)"""
    b = torch.zeros(8, C_)
    b[0] = b[2] = b[6] = 1.0
    return b


def _live(shape, pixels, seed):
    """(N,H,W,C) NHWC fp32 of bf16 values, zero except at the flat pixel indices `pixels`"""
    N, H, W, C_ = shape
    t = torch.zeros(N * H * W, C_)
    t[pixels] = bf16r(O.det_uniform((len(pixels), C_), seed))
    return t.view(N, H, W, C_)


def _plain_grad(t):
    g = L.MnasGradIn()
    g.g = t.data_ptr()
    return g


def _each_pixel_visible(contrib, bound, what):
    """every live pixel's own contribution exceeds the bound somewhere: dropping or doubling it would leave the bound"""
    for p, c in contrib:
        assert bool((c.abs() > 2 * bound).any()), "%s: the probe could not see pixel %d dropped" % (what, p)


@pytest.mark.parametrize("k", [1, 3])
def test_sparse_probe_conv_wgrad(k):
    """mnas_conv_wgrad (k_wgrad_t: 64-pixel chunks, split b owns pixels [b*chunk, (b+1)*chunk), chunk = 128 here), dense plain x,
    materialised dy live at 6 (1x1) / 12 (3x3: + image corners) pixels: check_sum_bound, c = 1, zero slack"""
    N, H, W, Ci, Co, nsplit = 2, 10, 10, 16, 24, 2
    M = N * H * W
    px = sorted({0, 63, 64, 127, 128, M - 1} | ({W - 1, (H - 1) * W, H * W - 1, H * W, H * W + W - 1, M - W} if k > 1 else set()))
    x = _nh(_x((N, Ci, H, W), 1)).contiguous()
    dy = _live((N, H, W, Co), px, 2)
    xd, dyd = x.to(torch.bfloat16).cuda(), dy.to(torch.bfloat16).cuda()
    got = _wgrad(N, H, W, Ci, H, W, Co, k, 1, k // 2, act_in(xd), _plain_grad(dyd), nsplit)
    r64, S, slack = wgrad_terms(Interval.exact(x, DEV), Interval.exact(dy, DEV), k, 1, k // 2, DEV)
    assert float(slack.max()) == 0.0
    what = "sparse conv_wgrad k%d" % k
    check_sum_bound(got.to(DEV), r64, S, M, nsplit, 1, what, None, "sparse probes")
    bound = (M + nsplit + 1) * 2.0 ** -22 * S
    def one(p):
        d1 = torch.zeros_like(dy)
        d1.view(M, Co)[p] = dy.view(M, Co)[p]
        return ref_dense_wgrad(x, d1, k, 1, k // 2, DEV)
    _each_pixel_visible([(p, one(p)) for p in px], bound, what)


def test_sparse_probe_pw_bwd():
    """mnas_pw_bwd in segment mode (workgroup b owns pixels [b*seg_px, (b+1)*seg_px)): dW and the fused reduce with g live at the
    first / last pixel and on both sides of the first tile and the first segment boundary; x read through the identity (1, 0)
    (act = relu(x) exactly), dy through the identity coefficients (dy = g exactly).  check_sum_bound c = 1 (zero slack) and
    check_red_bound (gin is zero off the live pixels)."""
    lib = L.load()
    Ci, Co = 32, 16
    tile = lib.mnas_pw_bwd_tile_pixels(Ci, Co)
    assert tile in (64, 128)
    seg = tile + tile // 2
    M = 2 * seg + 37
    nparts = (M + seg - 1) // seg
    px = sorted({0, tile - 1, tile, seg - 1, seg, M - 1})
    bx, b = _ident_bn(Ci), _ident_bn(Co)
    x = off_hinge(bf16r(O.det_uniform((1, 1, M, Ci), 1)), bx[0], bx[1])
    g = _live((1, 1, M, Co), px, 2)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 1, 1), 2))
    xd, gd, yd = x.to(torch.bfloat16).cuda(), g.to(torch.bfloat16).cuda(), torch.ones((1, 1, M, Co), dtype=torch.bfloat16, device="cuda")
    bxd, bd = bx.cuda(), b.cuda()
    gin, gchk = guarded((1, 1, M, Ci), torch.bfloat16)
    wpart, wchk = guarded((nparts, Co, Ci), torch.float32)
    redp, rchk = guarded((2, Ci, nparts), torch.float32)
    c = L.MnasPwBwd()
    c.M, c.Ci, c.Co, c.nparts, c.seg_px = M, Ci, Co, nparts, seg
    c.x, c.dy = act_in(xd, bxd[0], bxd[1]), grad_in(gd, yd, bd)
    c.w, c.gin, c.wpartial = L.ptr(pack(w, L.PACK_DGRAD)), L.ptr(gin), L.ptr(wpart)
    c.red_partial, c.red_y, c.red_bn = L.ptr(redp), L.ptr(xd), L.ptr(bxd)
    L.check(lib.mnas_pw_bwd(C.byref(c), L.cur_stream()), "pw_bwd")
    for chk, n in ((gchk, "gin"), (wchk, "wpartial"), (rchk, "red_partial")):
        chk("sparse pw_bwd " + n)
    grad = torch.full((Co, Ci, 1, 1), float("nan"), device="cuda")
    L.check(lib.mnas_wgrad_finalize(wpart.data_ptr(), nparts, Co, Ci, 1, grad.data_ptr(), 0, L.cur_stream()))
    a = torch.relu(x)
    r64, S, slack = wgrad_terms(Interval.exact(a, DEV), Interval.exact(g, DEV), 1, 1, 0, DEV)
    check_sum_bound(grad, r64, S, M, nparts, 1, "sparse pw_bwd dW", None, "sparse probes")
    _each_pixel_visible([(p, torch.outer(g.view(M, Co)[p], a.view(M, Ci)[p]).view(Co, Ci, 1, 1).to(DEV)) for p in px],
                        (M + nparts + 1) * 2.0 ** -22 * S, "sparse pw_bwd dW")
    dead = torch.ones(M, dtype=torch.bool)
    dead[px] = False
    assert not bool(gin.view(M, Ci)[dead.cuda()].any()), "gin of a pixel with dy = 0 is not zero"
    check_red_bound(redp, gin.float(), xd.float(), bx, M, "sparse pw_bwd", "sparse probes")


def _dw_probe_case(N, H, W, C_, k, which):
    """live dy pixels for a depthwise sweep of launch form `which` (as mnas_dw_rows): image corners (first and last pixel among
    them), both sides of the first strip boundary (column 4*sx) on both sides of the first DMA row-group boundary"""
    lib = L.load()
    geo = (C.c_int * 7)()
    assert lib.mnas_dw_geometry(N, H, W, C_, k, which, geo) == 0
    tw, strips, G_ = 4 * geo[1], geo[3], geo[6]
    rb = next(r for r in range(G_ - k // 2, H, G_) if r >= 1)     # groups start at row -PAD: first boundary inside the image (rows rb-1 | rb)
    assert strips >= 2 and 0 < tw < W and 0 < rb < H, (tw, strips, G_)
    at = lambda n, h, w_: (n * H + h) * W + w_
    px = {at(n, h, w_) for n in range(N) for h in (0, H - 1) for w_ in (0, W - 1)}
    px |= {at(0, h, w_) for h in (rb - 1, rb) for w_ in (tw - 1, tw)}
    return sorted(px)


@pytest.mark.parametrize("phase,k", [(0, 3), (2, 5)])
def test_sparse_probe_dw_bwd(phase, k):
    """mnas_dw_bwd phase 0 (fused: dW and reduce checked) and phase 2 (dW): g live at the image corners and around the first strip /
    row-group boundary (mnas_dw_geometry), x dense through the identity (1, 0), dy = g through the identity coefficients.
    check_sum_bound c = 2 (zero slack), check_red_bound."""
    lib = L.load()
    N, H, W, C_ = 2, 9, 20, 144
    which = 1 if phase == 0 else 3
    px = _dw_probe_case(N, H, W, C_, k, which)
    bx, b = _ident_bn(C_), _ident_bn(C_)
    x = off_hinge(bf16r(O.det_uniform((N, H, W, C_), 1)), bx[0], bx[1])
    g = _live((N, H, W, C_), px, 2)
    w = O.det_param("t.conv.weight", (C_, 1, k, k), 2)
    xd, gd = x.to(torch.bfloat16).cuda(), g.to(torch.bfloat16).cuda()
    yd = torch.ones((N, H, W, C_), dtype=torch.bfloat16, device="cuda")
    bxd, bd = bx.cuda(), b.cuda()
    nparts = 37
    rows = lib.mnas_dw_rows(N, H, W, C_, k, nparts, which)
    assert rows >= 2
    gin, gchk = guarded((N, H, W, C_), torch.bfloat16)
    wpart, wchk = guarded((rows, k * k, C_), torch.float32)
    redp, rchk = guarded((2, C_, rows), torch.float32)
    d = L.MnasDwBwd()
    d.N, d.H, d.W, d.C, d.k, d.nparts, d.phase = N, H, W, C_, k, nparts, phase
    d.x, d.dy = act_in(xd, bxd[0], bxd[1]), grad_in(gd, yd, bd)
    d.w, d.gin, d.wpartial = L.ptr(pack(w, L.PACK_DW)), L.ptr(gin), L.ptr(wpart)
    if phase == 0:
        d.red_bn, d.red_partial = L.ptr(bxd), L.ptr(redp)
    L.check(lib.mnas_dw_bwd(C.byref(d), L.cur_stream()), "dw_bwd")
    what = "sparse dw_bwd phase %d k%d" % (phase, k)
    wchk(what + " wpartial")
    grad = torch.full((C_, k, k), float("nan"), device="cuda")
    L.check(lib.mnas_dw_wgrad_finalize(wpart.data_ptr(), rows, C_, k, grad.data_ptr(), 0, L.cur_stream()))
    r64, S, slack = dw_wgrad_terms(Interval.exact(torch.relu(x), DEV), Interval.exact(g, DEV), k, 1, DEV)
    check_sum_bound(grad, r64, S, N * H * W, rows, 2, what + " dW", None, "sparse probes")
    if phase == 0:
        gchk(what + " gin")
        rchk(what + " red_partial")
        check_red_bound(redp, gin.float(), xd.float(), bx, N * H * W, what, "sparse probes")


def test_sparse_probe_conv_gemm_statistics():
    """statistics of mnas_conv_gemm mode 0 (1x1, plain x, no bias, two workgroups): x live at the first / last pixel and on both
    sides of the first two tile boundaries; every other output element must be exactly zero, check_stats_bound"""
    lib = L.load()
    Ci, Co = 48, 16
    tile = lib.mnas_conv_gemm_tile_pixels(2 * 128 + 37, Co, Ci)
    assert tile in (64, 128)
    M = 2 * tile + 37
    assert lib.mnas_conv_gemm_tile_pixels(M, Co, Ci) == tile
    px = sorted({0, tile - 1, tile, 2 * tile - 1, 2 * tile, M - 1})
    x = _live((1, 1, M, Ci), px, 1)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 1, 1), 2))
    xd = x.to(torch.bfloat16).cuda()
    out, st = conv_gemm(0, 1, 1, M, Ci, 1, M, Co, 1, 1, 0, pack(w, L.PACK_FWD), None, act=act_in(xd), nparts=2, stats=True, guard=True)
    r64, slack, S = onload_fwd_terms(Interval.exact(x, DEV), w, None, device=DEV)
    check_onload_bound(out, r64, slack, S, Ci, "sparse conv_gemm", "sparse probes: elements")
    dead = torch.ones(M, dtype=torch.bool, device="cuda")
    dead[px] = False
    assert not bool(out.view(M, Co)[dead].any())
    check_stats_bound(st, r64, onload_elem_err(slack, S, Ci), M, "sparse conv_gemm", "sparse probes")


def test_sparse_probe_dw_fwd_statistics():
    """statistics of mnas_dw_fwd (plain x, no bias, fp32 weights): x live at the image corners and around the first strip /
    row-group boundary; check_dw_bound and check_stats_bound"""
    lib = L.load()
    N, H, W, C_, k = 2, 9, 20, 144, 5
    px = _dw_probe_case(N, H, W, C_, k, 0)
    x = _live((N, H, W, C_), px, 1)
    w = O.det_param("t.conv.weight", (C_, 1, k, k), 2)
    xd = x.to(torch.bfloat16).cuda()
    nparts = 40
    rows = lib.mnas_dw_rows(N, H, W, C_, k, nparts, 0)
    assert rows >= 2
    out, ochk = guarded((N, H, W, C_), torch.bfloat16)
    st, schk = guarded((2, C_, rows), torch.float32)
    f = L.MnasDwFwd()
    f.N, f.H, f.W, f.C, f.k, f.nparts = N, H, W, C_, k, nparts
    f.in_ = act_in(xd)
    f.w, f.out, f.stats = L.ptr(pack(w, L.PACK_DW)), L.ptr(out), L.ptr(st)
    L.check(lib.mnas_dw_fwd(C.byref(f), L.cur_stream()), "dw_fwd")
    ochk("sparse dw_fwd out")
    schk("sparse dw_fwd stats")
    r64, S = dw_fwd_terms(Interval.exact(x, DEV), w.view(C_, k, k), None, 1, DEV)
    check_dw_bound(out, r64, S, k, "sparse dw_fwd", "sparse probes: elements")
    check_stats_bound(st, r64, dw_elem_err(S, k), N * H * W, "sparse dw_fwd", "sparse probes")


# ---------------------------------------------------------------------------------------------------
# stem input gradient on its own (no forward / weight-gradient launch: those take 16 and 32 couts here), pooling glue, and the
# sparse probes of the stem gradients and of mnas_pool_act
def _stem_dgrad(g, yd, bd, w32, N, H, W, Co, aff):
    lib = L.load()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dx, chk = guarded((N, 3, H, W), torch.float32)
    affd = aff.cuda().contiguous() if aff is not None else None
    gi = grad_in(g, yd, bd)
    L.check(lib.mnas_stem_dgrad(C.byref(gi), w32.data_ptr(), N, H, W, Ho, Wo, Co, L.ptr(affd), dx.data_ptr(), L.cur_stream()), "stem_dgrad")
    chk("stem_dgrad dx")
    return dx


@pytest.mark.parametrize("shape", [(2, 9, 11, 8), (1, 10, 12, 128), (6, 1, 1, 16), (3, 2, 7, 32)])
def test_stem_dgrad(shape):
    """mnas_stem_dgrad at 8 and 128 couts (the ends of what it takes), a 1x1 image (one contributing pixel, one tap) and odd /
    even sizes, fp32 weights that are not bf16 values: every element inside stem_dgrad_terms' bound, with and without in_affine"""
    N, H, W, Co = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    b = rand_bn_coefs(Co, 9, O)
    g, y = _x((N, Co, Ho, Wo), 6), _xoff((N, Co, Ho, Wo), 7, b[0], b[1])
    w_raw = O.det_param("t.conv.weight", (Co, 3, 3, 3), 2)
    w = bf16r(w_raw)
    assert not torch.equal(w, w_raw)
    gd, yd, bd, w32 = nhwc(g), nhwc(y), b.cuda(), w_raw.cuda().contiguous()
    div = dy_interval(_nh(g), _nh(y), b, True, DEV)
    for aff in (None, torch.tensor([[2.0, 0.5, 1.25], [0.1, 0.2, 0.3]])):
        dx = _stem_dgrad(gd, yd, bd, w32, N, H, W, Co, aff)
        r64, bound = stem_dgrad_terms(div, w, H, W, aff, DEV)
        r = _assert_bound(dx, r64, bound, "stem_dgrad %s affine %d" % (shape, aff is not None), "stem input gradient")
        print("stem_dgrad %s error / bound %.3f" % (shape, r))


def test_sparse_probe_stem_dgrad():
    """dy live at the four corners of the output plane of both images and at one interior pixel of each row / column parity (dy = g
    through the identity coefficients); odd H (the last output row's footprint ends at the last image row), even W.  dx inside
    stem_dgrad_terms' bound, exactly zero outside the live pixels' 3x3 footprints, and each live pixel visible."""
    N, H, W, Co = 2, 9, 10, 16
    Ho, Wo = 5, 5
    at = lambda n, h, w_: (n * Ho + h) * Wo + w_
    px = sorted({at(n, h, w_) for n in range(N) for h in (0, Ho - 1) for w_ in (0, Wo - 1)} | {at(0, 1, 2), at(0, 2, 1), at(1, 1, 1), at(1, 2, 2)})
    g = _live((N, Ho, Wo, Co), px, 2)
    b = _ident_bn(Co)
    w_raw = O.det_param("t.conv.weight", (Co, 3, 3, 3), 2)
    w = bf16r(w_raw)
    gd, yd = g.to(torch.bfloat16).cuda(), torch.ones((N, Ho, Wo, Co), dtype=torch.bfloat16, device="cuda")
    dx = _stem_dgrad(gd, yd, b.cuda(), w_raw.cuda().contiguous(), N, H, W, Co, None)
    d = Interval.exact(g, DEV)
    r64, bound = stem_dgrad_terms(d, w, H, W, None, DEV)
    _assert_bound(dx, r64, bound, "sparse stem_dgrad", "sparse probes: elements")
    foot = ref_dense_dgrad((g.abs().sum(-1, keepdim=True) > 0).double(), torch.ones(1, 1, 3, 3), H, W, 2, 1, DEV)[..., 0] > 0
    assert 0 < int(foot.sum()) < foot.numel()
    assert not bool(dx.permute(0, 2, 3, 1)[~foot].any()), "dx is not exactly zero outside the live pixels' footprints"
    def one(p):
        d1 = torch.zeros_like(g)
        d1.view(-1, Co)[p] = g.view(-1, Co)[p]
        return ref_dense_dgrad(d1, w, H, W, 2, 1, DEV).permute(0, 3, 1, 2)
    _each_pixel_visible([(p, one(p)) for p in px], bound, "sparse stem_dgrad")


@pytest.mark.parametrize("Co", [32, 16])
def test_sparse_probe_stem_wgrad(Co):
    """mnas_stem_wgrad, 32 couts: the band kernel (bands of RB = 4 output rows, band i on workgroup i % nparts, the last band of
    each image 2 rows); 16 couts: the im2col staging of k_wgrad (workgroup b owns pixels [b*128, (b+1)*128): 128-pixel blocks).
    Dense image, dy = g (identity coefficients) live at the four corners of both images' output planes (the image boundary among
    them, and column Wo-1), on both sides of the first band resp. block boundary (which is also the first workgroup boundary) --
    across the row end and within one column -- and of the 64-pixel mark.  check_sum_bound, c = 1, zero slack; each pixel visible."""
    lib = L.load()
    N, H, W, nparts = 2, 20, 32, 4
    Ho, Wo = 10, 16
    M = N * Ho * Wo
    at = lambda n, h, w_: (n * Ho + h) * Wo + w_
    if Co == 32:
        assert lib.mnas_stem_parts(1, N, H, W, Co) == 6           # a band shape: 2 x ceil(10 / 4) bands, more than nparts
        RB = stem_wgrad_band_rows(W, Wo)
        assert RB == 4 and Ho % RB
        bnd = RB * Wo
    else:
        assert lib.mnas_stem_parts(1, N, H, W, Co) == -1
        bnd = ((M + nparts - 1) // nparts + 127) // 128 * 128
        assert bnd == 128 and 2 * bnd < M
    px = {at(n, h, w_) for n in range(N) for h in (0, Ho - 1) for w_ in (0, Wo - 1)}
    px |= {bnd - 1, bnd, bnd - Wo + 5, bnd + 5, 63, 64, at(0, Ho - 1, 7), at(1, Ho - 2, 9)}
    px = sorted(px)
    x = bf16r(O.det_uniform((N, 3, H, W), 1))
    g = _live((N, Ho, Wo, Co), px, 2)
    gd, yd, bd = g.to(torch.bfloat16).cuda(), torch.ones((N, Ho, Wo, Co), dtype=torch.bfloat16, device="cuda"), _ident_bn(Co).cuda()
    xd = x.cuda()
    partial, pchk = guarded((nparts, Co, 27), torch.float32)
    s = L.MnasStemWgrad()
    s.N, s.H, s.W, s.Ho, s.Wo, s.Co, s.nparts = N, H, W, Ho, Wo, Co, nparts
    s.x, s.dy, s.partial = xd.data_ptr(), grad_in(gd, yd, bd), partial.data_ptr()
    L.check(lib.mnas_stem_wgrad(C.byref(s), L.cur_stream()), "stem_wgrad")
    pchk("sparse stem_wgrad partial")
    grad = torch.full((Co, 3, 3, 3), float("nan"), device="cuda")
    L.check(lib.mnas_wgrad_finalize(partial.data_ptr(), nparts, Co, 27, 1, grad.data_ptr(), 0, L.cur_stream()))
    r64, S, slack = wgrad_terms(Interval.exact(_nh(x), DEV), Interval.exact(g, DEV), 3, 2, 1, DEV)
    assert float(slack.max()) == 0.0
    what = "sparse stem_wgrad Co %d" % Co
    check_sum_bound(grad, r64, S, M, nparts, 1, what, None, "sparse probes")
    def one(p):
        d1 = torch.zeros_like(g)
        d1.view(M, Co)[p] = g.view(M, Co)[p]
        return ref_dense_wgrad(_nh(x), d1, 3, 2, 1, DEV)
    _each_pixel_visible([(p, one(p)) for p in px], sum_bound(S, M, nparts, 1), what)


@pytest.mark.parametrize("shape", [(2, 49, 320), (1, 1, 8), (2, 196, 1152), (3, 9, 8)])     # (N, HW, C)
@pytest.mark.parametrize("virt", [True, False])
def test_pool_act(shape, virt):
    """mnas_pool_act: R = 256 / (C / 8) row lanes, 8 loads per lane and batch pass.  (2, 49, 320): R = 6, the second pass holds one
    pixel; (1, 1, 8); (2, 196, 1152): R = 1; (3, 9, 8): R = 256 > HW.  Dense: every output inside pool_act_terms' bound
    (check_sum_bound's sum, then the division).  Sparse: pixels 0, R-1, R, 8R-1, 8R, HW-1 live where they exist -- virtual through
    the identity (1, 0), under which relu(0) = 0 keeps the others silent -- and each live pixel visible."""
    lib = L.load()
    N, HW, C_ = shape
    R = 256 // (C_ // 8)
    x = bf16r(O.det_uniform((N, HW, C_), 61))
    s, t = 1 + 0.3 * O.det_uniform((C_,), 62), 0.2 * O.det_uniform((C_,), 63)
    px = sorted({p for p in (0, R - 1, R, 8 * R - 1, 8 * R, HW - 1) if 0 <= p < HW})
    xs = torch.zeros_like(x)
    xs[:, px] = x[:, px]
    one, zero = torch.ones(C_), torch.zeros(C_)
    for what, xin, sc, sh in (("dense", x, s, t), ("sparse", xs, one, zero)):
        xd, sd, td = xin.to(torch.bfloat16).cuda(), sc.cuda(), sh.cuda()
        A = act_in(xd, sd, td) if virt else act_in(xd)
        out, chk = guarded((N, C_), torch.float32)
        L.check(lib.mnas_pool_act(C.byref(A), N, HW, C_, L.ptr(out), L.cur_stream()), "pool_act")
        what = "pool_act %s virt %d %s" % (shape, virt, what)
        chk(what)
        aiv = act_interval(xin, sc, sh, False, DEV) if virt else Interval.exact(xin, DEV)
        ref, bound = pool_act_terms(aiv, HW)
        r = _assert_bound(out, ref, bound, what, "pool_act" if xin is x else "sparse probes")
        print(what, "error / bound %.3f" % r)
    a = torch.relu(xs) if virt else xs
    _each_pixel_visible([(p, (a[:, p] / HW).to(DEV)) for p in px], bound, what)
