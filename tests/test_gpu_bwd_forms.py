"""-m gpu: the backward launches the engine makes by default, each kernel called on its own through the C ABI.

Part 1 (small and medium shapes, CPU fp64 references): the transposed-convolution input gradient of the stride-2 dense 3x3
convs (k_tcx<1,3>, k_tcx<2,5>, k_tcr, k_tconv), dy materialisation, the merged BatchNorm / weight-gradient finalize
(k_bwd_post), the production forms of the fused 1x1 backward (RECOMP, gin_masked, segment mode) and the fused depthwise
backward on a masked gradient.  Part 2: the distinct launches of the bench configuration's training Program (bs 256, 224x224)
replayed standalone with the production integers against fp64 references computed on the device.

Every output and partial table lives in a guarded buffer (tests/gpu_util.py): a write outside it, or an element never written,
fails the test.  On top of the max-normalised tolerances every launch is held to the derived bounds of tests/bounds_conv.py: the
input gradients element by element (check_onload_bound over the dy-on-load interval, check_dw_bound for the sweeps), the weight
gradients and fused reduces per element / channel (check_sum_bound, check_red_bound), the merged finalize launch per channel and
per weight (bn_bwd_finalize_intervals, check_sum_bound) and bit for bit to the standalone finalizes on the same tables.  Where include/mnas.h promises bit-identical results (RECOMP vs the stored y, masked vs plain gradients, grid
size), the comparison is bit for bit and names the first differing element."""
import ctypes as C

import pytest
import torch

from cases import O
from bounds_conv import (HINGE, act_interval, check_dw_bound, check_onload_bound, check_red_bound, dw_dgrad_terms, dw_wgrad_terms,
                         dy_interval, off_hinge, onload_dgrad_terms, relu_mask, zero_on_hinge)
from bounds_se import bn_bwd_finalize_intervals
from gpu_util import L, act_in, bf16r, bits_equal, conv_gemm, grad_in, guarded, pack, rand_bn_coefs, relerr
from intervals import Interval, check_interval, check_sum_bound
from refs64 import ref_dense_dgrad, ref_dw_dgrad, ref_dw_wgrad, ref_dy
from test_gpu_kernels import DW, PWB, TOL_BF16, TOL_F32

pytestmark = pytest.mark.gpu
TOL_RED = 1e-3          # fused BatchNorm-backward reduce sums (as test_pw_dgrad)
_off_hinge = off_hinge  # (bounds_conv: inputs are moved off the ReLU hinge |s*v+t| < HINGE, host and device then agree on every mask bit)
assert HINGE == 1e-3
BOUND_ELEMS = 16 << 20  # fp64 elements of one operand chunk of the per-element bounds


def _x(shape, seed):
    return bf16r(O.det_uniform(shape, seed))


def _cdiv(a, b):
    return (a + b - 1) // b


def _mask(v, s, t):
    return (s.double().to(v.device) * v.double() + t.double().to(v.device)) > 0


def _red_ref(gq, yin, bn):
    """fp64 (sum dz, sum dz*xhat) per channel of the fused reduce: gq, yin (..., C) as stored, bn = bnbuf [8][C]"""
    bn = bn.double().to(gq.device)
    gq, yin = gq.double(), yin.double()
    dz = gq * ((bn[0] * yin + bn[1]) > 0)
    xhat = (yin - bn[5]) * bn[6]
    dims = tuple(range(gq.dim() - 1))
    return dz.sum(dims), (dz * xhat).sum(dims)


def _check_red(table, gq, yin, bn, what):
    s1, s2 = _red_ref(gq, yin, bn)
    p = table.double().sum(-1)
    assert relerr(p[0], s1) < TOL_RED, (what, "sum dz", relerr(p[0], s1))
    assert relerr(p[1], s2) < TOL_RED, (what, "sum dz*xhat", relerr(p[1], s2))


# =====================================================================================================================================
# 1.1  mnas_tconv_dgrad: the input gradient of every stride-2 dense 3x3 with an even plane
# =====================================================================================================================================
def _tconv_parts_expected(kernel, N, Ho, Wo, Co, Ci):
    """what csrc/mnas_tconv.hip's dispatcher implies for the preferred grid of each kernel (tcx_plan / tcr_plan / tconv_ok)"""
    M2 = N * Ho * Wo
    if kernel == "tcx13":
        return min(_cdiv(M2, 16), 1024)
    if kernel == "tcx25":
        return min(_cdiv(M2, 16), 768)
    if kernel == "tcr":
        return min(max(1, 256 // (Ci // 16)), N)
    return min(_cdiv(M2, 64), 512)          # k_tconv, 64-pixel tiles: min(tiles, 256 CUs x 2 resident workgroups of 80.5 KB)


TCONV = [  # kernel, N, Ho, Wo (dy plane; the result plane is 2Ho x 2Wo), Co (dy channels), Ci (result channels)
    ("tcx13", 2, 56, 56, 24, 16), ("tcx13", 3, 13, 9, 24, 16),
    ("tcx25", 2, 28, 28, 40, 24), ("tcx25", 5, 7, 11, 40, 32), ("tcx25", 2, 28, 28, 40, 32), ("tcx25", 5, 7, 11, 40, 24),
    ("tcr", 32, 7, 7, 192, 96), ("tcr", 33, 6, 7, 192, 112), ("tcr", 45, 8, 8, 192, 160), ("tcr", 33, 4, 5, 192, 96),
    ("tcr", 45, 7, 7, 192, 112),
    # k_tconv: what neither k_tcx (Co <= 40) nor k_tcr (Co = 192) takes and fits its 80 KB LDS budget -- 48 -> 8 channels
    ("tconv", 2, 9, 11, 48, 8), ("tconv", 3, 8, 7, 48, 8),
]


def _tconv_launch(lib, N, Ho, Wo, Co, Ci, dyd, wp, nparts, red=None):
    out, chk = guarded((N, 2 * Ho, 2 * Wo, Ci), torch.bfloat16)
    st, schk = (guarded((2, Ci, nparts), torch.float32) if red is not None else (None, None))
    a = L.MnasTconvDgrad()
    a.N, a.Ho, a.Wo, a.Co, a.Ci, a.nparts = N, Ho, Wo, Co, Ci, nparts
    a.dy, a.w, a.out = L.ptr(dyd), L.ptr(wp), L.ptr(out)
    if red is not None:
        a.stats, a.red_y, a.red_bn = L.ptr(st), L.ptr(red[0]), L.ptr(red[1])
    L.check(lib.mnas_tconv_dgrad(C.byref(a), L.cur_stream()), "tconv_dgrad")
    chk("tconv out (nparts %d)" % nparts)
    if schk is not None:
        schk("tconv stats (nparts %d)" % nparts)
    return out, st


@pytest.mark.parametrize("case", TCONV, ids=["%s_%dx%dx%d_%d_%d" % c for c in TCONV])
@pytest.mark.parametrize("fused_red", [False, True], ids=["plain", "red"])
def test_tconv_dgrad(case, fused_red):
    """+ check_onload_bound (materialised dy: the plain special case) and check_red_bound"""
    kernel, N, Ho, Wo, Co, Ci = case
    lib = L.load()
    H, W = 2 * Ho, 2 * Wo
    assert lib.mnas_tconv_supported(Ho, Wo, Co, Ci) == 1
    pref = lib.mnas_tconv_parts(N, Ho, Wo, Co, Ci)
    assert pref == _tconv_parts_expected(kernel, N, Ho, Wo, Co, Ci), (kernel, pref)
    if kernel == "tcr":      # k_tcr needs N >= 32: below that no kernel takes the shape (4*Ci > 96 rules out k_tconv)
        assert lib.mnas_tconv_parts(31, Ho, Wo, Co, Ci) == -1
    dy = _x((N, Ho, Wo, Co), 3)
    w = bf16r(O.det_param("t.conv.weight", (Co, Ci, 3, 3), 2))
    ref = ref_dense_dgrad(dy, w, H, W, stride=2, pad=1)
    dyd = dy.to(torch.bfloat16).cuda()
    wp = pack(w, L.PACK_TCONV)
    red = None
    if fused_red:
        b_in = rand_bn_coefs(Ci, 22, O)
        y_in = _off_hinge(_x((N, H, W, Ci), 21), b_in[0], b_in[1])
        red = (y_in.to(torch.bfloat16).cuda(), b_in.cuda())
    # per-element bound: dy is materialised (a zero-width interval), K = 9*Co bounds the accumulations of any output pixel
    r64, slack, S = onload_dgrad_terms(Interval.exact(dy, "cuda"), w, H, W, 2, 1, None, "cuda")
    outs = []
    for nparts in sorted({1, pref, pref + 7}):
        out, st = _tconv_launch(lib, N, Ho, Wo, Co, Ci, dyd, wp, nparts, red)
        outs.append((nparts, out))
        assert relerr(out.double().cpu(), ref) < TOL_BF16, (kernel, nparts, relerr(out.double().cpu(), ref))
        check_onload_bound(out, r64, slack, S, 9 * Co, "tconv %s nparts %d" % (kernel, nparts), "transposed-conv input gradient")
        if fused_red:
            _check_red(st.cpu(), out.float().cpu(), y_in, b_in, "tconv %s nparts %d" % (kernel, nparts))
            check_red_bound(st, out.float(), red[0].float(), b_in, N * H * W, "tconv %s nparts %d" % (kernel, nparts), "fused reduce (GEMM)")
    for nparts, out in outs[1:]:
        bits_equal(out, outs[0][1], "tconv %s out, nparts %d vs %d" % (kernel, nparts, outs[0][0]))
    # the input-gradient GEMM the dispatcher replaced, on the same operands
    g = L.MnasGradIn()
    g.g = L.ptr(dyd)
    alt, _ = conv_gemm(1, N, Ho, Wo, Co, H, W, Ci, 3, 2, 1, pack(w, L.PACK_DGRAD), None, grad=g, nparts=64)
    assert relerr(alt.double().cpu(), outs[0][1].double().cpu()) < TOL_BF16


def test_tconv_dgrad_rejects():
    lib = L.load()
    dyd = torch.zeros((31, 7, 7, 192), dtype=torch.bfloat16, device="cuda")
    out = torch.zeros((31, 14, 14, 96), dtype=torch.bfloat16, device="cuda")
    a = L.MnasTconvDgrad()
    a.N, a.Ho, a.Wo, a.Co, a.Ci, a.nparts = 31, 7, 7, 192, 96, 8
    a.dy, a.w, a.out = L.ptr(dyd), L.ptr(dyd), L.ptr(out)
    assert lib.mnas_tconv_dgrad(C.byref(a), L.cur_stream()) == L.EINVAL          # k_tcr below N = 32
    a.N, a.Co, a.Ci, a.Ho, a.Wo = 2, 24, 16, 7, 7
    a.nparts = 0
    assert lib.mnas_tconv_dgrad(C.byref(a), L.cur_stream()) == L.EINVAL
    a.nparts = 4
    a.red_y = L.ptr(out)                                                          # reduce operand without bnbuf / stats
    assert lib.mnas_tconv_dgrad(C.byref(a), L.cur_stream()) == L.EINVAL


# =====================================================================================================================================
# 1.2  mnas_dy_materialize
# =====================================================================================================================================
def _check_dy_mat(out, g, y, coef, what):
    """out (bf16) within one bf16 ulp of bf16(fp64 formula).  The floor 2^-22 * (|c1 g| + |c2 y| + |c3|) covers results that
    cancel to far below their terms, where the kernel's fp32 arithmetic (not its bf16 store) sets the error."""
    ref = ref_dy(g, y, coef, device=out.device)
    cf = coef.double().to(out.device)
    scale = (cf[2] * g.double()).abs() + (cf[3] * y.double()).abs() + cf[4].abs()
    rq = ref.to(torch.bfloat16).double()
    _, e = torch.frexp(rq)
    ulp = torch.where(rq == 0, torch.zeros_like(rq), torch.ldexp(torch.ones_like(rq), (e - 8).to(torch.int32)))
    bound = torch.maximum(ulp, scale * 2.0 ** -22)
    err = (out.double() - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d elements off by more than one bf16 ulp; first %s: got %r, fp64 %r"
                             % (what, int(bad.sum()), idx, float(out[idx]), float(ref[idx])))


@pytest.mark.parametrize("C_,rows", [(8, 1001), (24, 333), (40, 4099), (72, 77), (1152, 195)])
def test_dy_materialize(C_, rows):
    lib = L.load()
    g, y = _x((rows, C_), 1), _x((rows, C_), 2)
    b = rand_bn_coefs(C_, 9, O)
    gd, yd, bd = g.to(torch.bfloat16).cuda(), y.to(torch.bfloat16).cuda(), b.cuda()
    out, chk = guarded((rows, C_), torch.bfloat16)
    gi = grad_in(gd, yd, bd)
    L.check(lib.mnas_dy_materialize(C.byref(gi), rows, C_, L.ptr(out), L.cur_stream()), "dy_materialize")
    chk("dy_materialize out")
    _check_dy_mat(out, gd, yd, bd, "dy_materialize C=%d rows=%d" % (C_, rows))
    assert bool(((b[0] * y + b[1]) <= 0).any()) and bool(((b[0] * y + b[1]) > 0).any())


# =====================================================================================================================================
# 1.3  mnas_bwd_post: BatchNorm-backward finalize + up to two weight-gradient reductions in one launch
# =====================================================================================================================================
def _post(lib, bn=None, w1=None, w2=None, expect=0):
    p = L.MnasBwdPost()
    if bn is not None:
        partial, bnbuf, dgamma, dbeta, nparts, C_, count = bn
        p.bn_partial, p.bnbuf, p.dgamma, p.dbeta = L.ptr(partial), L.ptr(bnbuf), L.ptr(dgamma), L.ptr(dbeta)
        p.count, p.bn_nparts, p.bn_C = count, nparts, C_
    for slot, w in (("w1", w1), ("w2", w2)):
        if w is not None:
            partial, grad, nsplit, Co, Ci, taps, dw, level = w
            t = getattr(p, slot)
            t.partial, t.grad = L.ptr(partial), L.ptr(grad)
            t.nsplit, t.Co, t.Ci, t.taps, t.dw, t.level = nsplit, Co, Ci, taps, dw, level
    rc = lib.mnas_bwd_post(C.byref(p), L.cur_stream())
    if expect:
        assert rc == expect, rc
    else:
        L.check(rc, "bwd_post")


FAMILY_POST = "fused finalize launch"


def _pow2_scale(n, lo=-20, hi=4, step=7):
    """n exact powers of two 2^lo .. 2^hi, in an order that puts unlike magnitudes next to each other"""
    k = (torch.arange(n) * step) % (hi - lo + 1) + lo
    return torch.pow(torch.tensor(2.0), k.float())


def _wg_live_rows(nsplit):
    """the sparse probe of the two-level reduction: the first row, the last, and both sides of every 128-row chunk boundary"""
    return sorted({r for r in [0, nsplit - 1] + [b + d for b in range(128, nsplit, 128) for d in (-1, 0)] if 0 <= r < nsplit})


class _Wg:
    """one weight-gradient reduction task: guarded partial table and accumulation target; fp64 expectation.  table: "uniform"
    (det_uniform); "scaled": rows and columns times powers of two 2^-20..2^4; "sparse": zero but for the rows of _wg_live_rows,
    whose entries are bounded away from zero (0.5..1 in magnitude), so that every live term exceeds twice the bound."""
    def __init__(self, nsplit, Co, Ci, taps, dw, seed, table="uniform"):
        self.nsplit, self.Co, self.Ci, self.taps, self.dw, self.table = nsplit, Co, Ci, taps, dw, table
        shape = (nsplit, taps, Co) if dw else (nsplit, Co, taps * Ci)
        gshape = (Co, taps) if dw else (Co, Ci, taps)
        self.part_host = O.det_uniform(shape, seed)
        self.init = O.det_uniform(gshape, seed + 1)
        if table == "scaled":
            cols = shape[1] * shape[2]
            self.part_host = self.part_host * _pow2_scale(nsplit).view(-1, 1, 1) * _pow2_scale(cols, step=11).view(1, shape[1], shape[2])
            self.init = self.init * _pow2_scale(self.init.numel(), step=3).view(gshape)
        elif table == "sparse":
            live = torch.zeros(nsplit, dtype=torch.bool)
            live[_wg_live_rows(nsplit)] = True
            u = self.part_host
            self.part_host = torch.where(live.view(-1, 1, 1), torch.sign(u + 1e-9) * (0.5 + 0.5 * u.abs()), torch.zeros_like(u))
            self.init = torch.zeros(gshape)
        else:
            assert table == "uniform"
        self.part, self.pchk = guarded(shape, torch.float32)
        self.part.copy_(self.part_host.cuda())
        self.grad, self.gchk = guarded(gshape, torch.float32)
        self.grad.copy_(self.init.cuda())
        S = self.part_host.double().sum(0)
        self.want = self._lay(S) + self.init.double()
        self.mag = self._lay(self.part_host.double().abs().sum(0)) + self.init.double().abs()

    def _lay(self, S):
        return S.t() if self.dw else S.view(self.Co, self.taps, self.Ci).permute(0, 2, 1)

    def slot(self, level):
        return (self.part, self.grad, self.nsplit, self.Co, 1 if self.dw else self.Ci, self.taps, self.dw, level)

    def check(self, what):
        """+ check_sum_bound: M = nsplit terms, c = 1, the accumulate target is the +1; level 2 then 3 (more than 256 rows): P =
        the number of 128-row chunks the second level adds.  + bit equality with the standalone finalize on the same table (the same template
        instances: k_wgrad_finalize<DW, false> up to 256 rows, <DW, true> then <DW, false> above)."""
        self.pchk(what + " partial")
        self.gchk(what + " grad")
        assert relerr(self.grad.cpu(), self.want) < 1e-5, (what, relerr(self.grad.cpu(), self.want))
        P = _cdiv(self.nsplit, 128) if self.nsplit > 256 else 0
        r = check_sum_bound(self.grad.cpu(), self.want, self.mag, self.nsplit, P, 1, what + " (%s table)" % self.table, None, FAMILY_POST)
        if self.table == "sparse":
            bound = (self.nsplit + P + 1) * 2.0 ** -22 * self.mag
            for row in _wg_live_rows(self.nsplit):
                assert bool((self._lay(self.part_host[row].double().abs()) > 2 * bound).all()), (what, "live row %d would not be seen" % row)
            print("%s: sparse probe error / bound %.3f" % (what, r))
        lib = L.load()
        p2, g2 = self.part_host.clone().cuda(), self.init.clone().cuda()
        if self.dw:
            k = int(round(self.taps ** 0.5))
            L.check(lib.mnas_dw_wgrad_finalize(L.ptr(p2), self.nsplit, self.Co, k, L.ptr(g2), 1, L.cur_stream()), "dw_wgrad_finalize")
        else:
            L.check(lib.mnas_wgrad_finalize(L.ptr(p2), self.nsplit, self.Co, self.Ci, self.taps, L.ptr(g2), 1, L.cur_stream()), "wgrad_finalize")
        bits_equal(self.grad, g2, what + ": fused launch vs the standalone finalize")
        return r


def _bn_table(C_, nparts, seed, b, table):
    """the [2][C][nparts] table of (sum dz, sum dz*xhat) partials.  "uniform": det_uniform.  "hard": every channel times a power
    of two 2^-20..2^4 and every partial column times 2^0..2^-7; in channels c % 3 == 1 the sum dz partials are mean*invstd times
    the sum dz*xhat ones (rounded to fp32), so that row 4 = s (mean invstd S2 - S1) / count cancels; the last channel (C > 1) is
    exact zeros."""
    p = O.det_uniform((2, C_, nparts), seed)
    if table == "uniform":
        return p
    assert table == "hard"
    p = p * _pow2_scale(C_).view(1, -1, 1) * _pow2_scale(nparts, -7, 0, 3).view(1, 1, -1)
    c = torch.arange(C_) % 3 == 1
    p[0, c] = ((b[5] * b[6])[c].double().view(-1, 1) * p[1, c].double()).float()
    if C_ > 1:
        p[:, C_ - 1] = 0.0
    return p


def _bn_task(C_, nparts, seed, table="uniform"):
    b = rand_bn_coefs(C_, seed + 1, O)
    partial = _bn_table(C_, nparts, seed, b, table)
    bp, pchk = guarded((2, C_, nparts), torch.float32)
    bp.copy_(partial.cuda())
    bnbuf, bchk = guarded((8, C_), torch.float32)
    bnbuf.copy_(b.cuda())
    dg, dgchk = guarded((C_,), torch.float32)
    db, dbchk = guarded((C_,), torch.float32)
    g0, b0 = O.det_uniform((C_,), seed + 2), O.det_uniform((C_,), seed + 3)
    dg.copy_(g0.cuda())
    db.copy_(b0.cuda())
    count = 12345.0
    S = partial.double().sum(-1)

    def check(what):
        for c, n in ((pchk, "bn partial"), (bchk, "bnbuf"), (dgchk, "dgamma"), (dbchk, "dbeta")):
            c("%s %s" % (what, n))
        assert relerr(dg.cpu(), g0.double() + S[1]) < 1e-5 and relerr(db.cpu(), b0.double() + S[0]) < 1e-5, what
        # rows 2..4 as the standalone finalize writes them (same partial table, accumulate = 1)
        bn2 = b.clone().cuda()
        dg2, db2 = g0.clone().cuda(), b0.clone().cuda()
        L.check(L.load().mnas_bn_bwd_finalize(L.ptr(bp), nparts, C_, count, L.ptr(bn2), L.ptr(dg2), L.ptr(db2), 1, L.cur_stream()))
        got = bnbuf.cpu().double()
        for r in (2, 3, 4):
            assert relerr(got[r], bn2[r].cpu().double()) < 1e-6, (what, "bnbuf row", r)
        for r in (0, 1, 5, 6):
            assert torch.equal(got[r], b[r].double()), (what, "bnbuf row %d changed" % r)
        # every channel inside the brackets of the table as given (fp64 on the fp32 partials; bounds_se.bn_bwd_finalize_intervals)
        ivs = bn_bwd_finalize_intervals(partial, count, b, g0, b0)
        fin = {"c1": bnbuf[2], "c2": bnbuf[3], "c3": bnbuf[4], "dgamma": dg, "dbeta": db}
        worst = max(check_interval(fin[k].cpu(), iv, "%s %s (%s table)" % (what, k, table), FAMILY_POST) for k, iv in ivs.items())
        # ... and the standalone's bits: bn_bwd_finalize_body<64> up to 256 partials, <256> above, in both launches
        bits_equal(bnbuf[2:5], bn2[2:5], what + ": rows 2..4, fused launch vs mnas_bn_bwd_finalize")
        bits_equal(dg, dg2, what + ": dgamma, fused launch vs mnas_bn_bwd_finalize")
        bits_equal(db, db2, what + ": dbeta, fused launch vs mnas_bn_bwd_finalize")
        return worst
    return (bp, bnbuf, dg, db, nparts, C_, count), check, (bnbuf, dg, db)


@pytest.mark.parametrize("C_", [24, 1152])
@pytest.mark.parametrize("bn_nparts", [7, 256, 257, 1031])
def test_bwd_post_bn(C_, bn_nparts):
    """the BatchNorm part alone, on both sides of bn_wide (nparts > 256: one block per channel)"""
    lib = L.load()
    bn, check, _ = _bn_task(C_, bn_nparts, 60)
    _post(lib, bn=bn)
    check("bwd_post bn C=%d nparts=%d" % (C_, bn_nparts))


@pytest.mark.parametrize("dw", [0, 1], ids=["dense", "dw"])
@pytest.mark.parametrize("nsplit", [1, 128, 256])
def test_bwd_post_level1(dw, nsplit):
    lib = L.load()
    Co, Ci, taps = (72, 1, 9) if dw else (40, 24, 9)
    w1 = _Wg(nsplit, Co, Ci, taps, dw, 70)
    _post(lib, w1=w1.slot(1))
    w1.check("level 1 w1 only")
    # w1 + w2 (the second a 1x1 / 5x5 table) + the BatchNorm part in one launch
    w1 = _Wg(nsplit, Co, Ci, taps, dw, 72)
    w2 = _Wg(max(1, nsplit - 1), 48, 16, 1, 0, 74) if not dw else _Wg(max(1, nsplit - 1), 40, 1, 25, 1, 74)
    bn, check, _ = _bn_task(40, 33, 76)
    _post(lib, bn=bn, w1=w1.slot(1), w2=w2.slot(1))
    w1.check("level 1 w1 (+w2, bn)")
    w2.check("level 1 w2 (+w1, bn)")
    check("level 1 bn (+w1, w2)")


@pytest.mark.parametrize("dw", [0, 1], ids=["dense", "dw"])
@pytest.mark.parametrize("nsplit", [257, 300, 1024, 1025])
def test_bwd_post_level2_then_3(dw, nsplit):
    """two-level reduction as the engine queues it: level 2 (fold 128-row chunks in place) beside another layer's work, level 3
    in a LATER launch; both launches also carry a second task and a BatchNorm part.  Two identical runs are bit-identical."""
    lib = L.load()
    Co, Ci, taps = (40, 1, 25) if dw else (16, 48, 1)
    grads = []
    for rep in range(2):
        w = _Wg(nsplit, Co, Ci, taps, dw, 80)
        other = _Wg(3, 24, 8, 9, 0, 82)
        bn, check, _ = _bn_task(48, 300, 84)
        _post(lib, bn=bn, w1=w.slot(2), w2=other.slot(1))
        other.check("level 2 launch: w2")
        check("level 2 launch: bn")
        other2 = _Wg(130, 16, 1, 9, 1, 86)
        _post(lib, w1=other2.slot(1), w2=w.slot(3))
        w.check("level 3 (nsplit %d)" % nsplit)
        other2.check("level 3 launch: w1")
        grads.append(w.grad.clone())
    bits_equal(grads[1], grads[0], "bwd_post level 2+3 rerun")


def test_bwd_post_level0_slots_and_rejects():
    lib = L.load()
    w2 = _Wg(5, 24, 16, 9, 0, 90)
    _post(lib, w1=(None, None, 0, 0, 0, 0, 0, 0), w2=w2.slot(1))          # w1 empty, w2 live
    w2.check("w1 level 0, w2 level 1")
    bn, check, _ = _bn_task(16, 7, 92)
    _post(lib, bn=bn)                                                       # both slots level 0
    check("bn with both slots at level 0")
    _post(lib)                                                              # nothing at all: no launch, OK
    bad = _Wg(257, 8, 8, 1, 0, 94)
    _post(lib, w1=bad.slot(1), expect=L.EINVAL)                             # single level only up to 256 rows
    _post(lib, w1=bad.slot(4), expect=L.EINVAL)
    _post(lib, w2=bad.slot(1), expect=L.EINVAL)
    bad.pchk("rejected launches: partial", written=True)
    assert torch.equal(bad.grad.cpu(), bad.init), "a rejected launch wrote the gradient"


@pytest.mark.parametrize("C_", [1, 3, 4, 5])
@pytest.mark.parametrize("bn_nparts", [1, 256, 257, 1025])
def test_bwd_post_mapping(C_, bn_nparts):
    """the mapping of workgroups to the three parts, with tables that can go wrong.  The BatchNorm part (a hard table: scales
    2^-20..2^4, cancelling channels, a channel of zeros; C = 1, 3, 4, 5: a partial last workgroup of the four-channels-per-
    workgroup form, one workgroup per channel above 256 partials; 1025 partials: two terms per fp32 accumulator) runs beside
    w1 alone, beside w2 alone (w1 at level 0), and beside both -- three parts of different sizes (108, 5 and 24 x 3 workgroups)
    -- at level 1 and at level 2 then 3 with the two-level task in either slot.  Every output inside its bracket and bit-equal
    to the standalone finalize's."""
    lib = L.load()
    what = "mapping C=%d nparts=%d" % (C_, bn_nparts)
    empty = (None, None, 0, 0, 0, 0, 0, 0)
    A = lambda tab="scaled": _Wg(5, 24, 16, 9, 0, 110, tab)             # 3456 outputs: 108 workgroups
    B = lambda tab="scaled": _Wg(130, 16, 1, 9, 1, 112, tab)            # 144 outputs: 5 workgroups
    T2 = lambda tab="sparse": _Wg(300, 16, 48, 1, 0, 114, tab)          # 768 outputs: 24 x 3 workgroups at level 2, 24 at level 3
    worst = 0.0
    for name, slots in (("w1 only", lambda a, b: dict(w1=a.slot(1))), ("w2 only", lambda a, b: dict(w1=empty, w2=b.slot(1))),
                        ("w1 + w2", lambda a, b: dict(w1=a.slot(1), w2=b.slot(1))), ("w2 + w1", lambda a, b: dict(w1=b.slot(1), w2=a.slot(1)))):
        a, b = A(), B()
        bn, check, _ = _bn_task(C_, bn_nparts, 120, "hard")
        kw = slots(a, b)
        _post(lib, bn=bn, **kw)
        worst = max(worst, check("%s, %s: bn" % (what, name)))
        for w in (a, b):
            if any(v is not None and v is not empty and v[0] is w.part for v in kw.values()):
                worst = max(worst, w.check("%s, %s: %s" % (what, name, "A" if w is a else "B")))
    for slot2, slot3 in (("w1", "w2"), ("w2", "w1")):
        for tab in ("sparse", "scaled"):
            w, a, b = T2(tab), A(), B()
            bn, check, _ = _bn_task(C_, bn_nparts, 122, "hard")
            _post(lib, bn=bn, **{slot2: w.slot(2), ("w2" if slot2 == "w1" else "w1"): a.slot(1)})
            worst = max(worst, check("%s, level 2 in %s: bn" % (what, slot2)), a.check("%s, level 2 in %s: A" % (what, slot2)))
            bn, check, _ = _bn_task(C_, bn_nparts, 124, "hard")
            _post(lib, bn=bn, **{slot3: w.slot(3), ("w2" if slot3 == "w1" else "w1"): b.slot(1)})
            worst = max(worst, check("%s, level 3 in %s: bn" % (what, slot3)), b.check("%s, level 3 in %s: B" % (what, slot3)),
                        w.check("%s, level 2 in %s then 3 in %s (%s)" % (what, slot2, slot3, tab)))
    print("%s: worst error / bound %.3f" % (what, worst))


@pytest.mark.parametrize("dw", [0, 1], ids=["dense", "dw"])
@pytest.mark.parametrize("nsplit", [1, 128, 129, 256, 257, 384, 385, 1025])
@pytest.mark.parametrize("table", ["scaled", "sparse"])
def test_bwd_post_tables(dw, nsplit, table):
    """the weight-gradient tasks alone on tables that can go wrong: rows and columns scaled by 2^-20..2^4, and the sparse probe (one
    live row first, last and on both sides of every 128-row chunk boundary); single level up to 256 rows, level 2 then 3 above"""
    lib = L.load()
    Co, Ci, taps = (40, 1, 25) if dw else (16, 12, 9)
    w = _Wg(nsplit, Co, Ci, taps, dw, 130, table)
    if nsplit <= 256:
        _post(lib, w2=w.slot(1))
    else:
        _post(lib, w1=w.slot(2))
        _post(lib, w1=w.slot(3))
    r = w.check("tables %s nsplit %d dw %d" % (table, nsplit, dw))
    print("bwd_post %s table nsplit %d dw %d: error / bound %.3f" % (table, nsplit, dw, r))


# =====================================================================================================================================
# 1.4  mnas_pw_bwd production forms
# =====================================================================================================================================
class _PwCase:
    """operands of one fused 1x1 backward: x (M,Ci) read through its producer's (scale, shift) when virtual, dy-on-load of (g, y)
    with this layer's coefficients, fp32 weights rounded to bf16 by the packer.  Device tensors; `gen` seeds them."""
    def __init__(self, M, Ci, Co, gen, virt=True, y=None, bias=False):
        dev = "cuda"
        self.M, self.Ci, self.Co, self.virt = M, Ci, Co, virt
        u = lambda *s: torch.rand(*s, generator=gen, device=dev) * 2 - 1
        self.bx = torch.zeros(8, Ci, device=dev)
        self.bx[0], self.bx[1] = 1 + 0.3 * u(Ci), 0.2 * u(Ci)
        self.bx[2], self.bx[3], self.bx[4] = self.bx[0], 0.05 * u(Ci), 0.02 * u(Ci)
        self.bx[5], self.bx[6] = 0.1 * u(Ci), 1 + 0.2 * u(Ci).abs()
        x = _off_hinge(bf16r(u(M, Ci)), self.bx[0], self.bx[1])      # (always: x feeds the fused reduce's mask)
        self.x = x.to(torch.bfloat16)
        self.b = torch.zeros(8, Co, device=dev)
        self.b[0], self.b[1] = 1 + 0.3 * u(Co), 0.2 * u(Co)
        self.b[2], self.b[3], self.b[4] = self.b[0], 0.05 * u(Co), 0.02 * u(Co)
        self.b[5], self.b[6] = 0.1 * u(Co), 1 + 0.2 * u(Co).abs()
        self.g = bf16r(u(M, Co)).to(torch.bfloat16)
        self.w = bf16r(u(Co, Ci) * (3.0 / Ci) ** 0.5)
        self.wd = pack(self.w.view(Co, Ci, 1, 1), L.PACK_DGRAD)
        self.bias = 0.1 * u(Co) if bias else None
        if y is None:
            y = _off_hinge(bf16r(u(M, Co)), self.b[0], self.b[1]).to(torch.bfloat16)
            self.y = y
        else:
            self.set_y(y)

    def set_y(self, y):
        """a y that another kernel wrote (the forward's stored output, for RECOMP) cannot be moved off the hinge: g is cleared there"""
        self.y = y
        self.g = zero_on_hinge(self.g, y, self.b[0], self.b[1])

    def act(self):
        a = self.x.double()
        if self.virt:
            a = bf16r(torch.relu(self.bx[0] * self.x.float() + self.bx[1])).double()
        return a

    def dy(self):
        return bf16r(ref_dy(self.g, self.y, self.b, device="cuda").float()).double()      # staged as bf16 for the MFMA

    def launch(self, nparts, red=True, recomp=None, masked=0, seg_px=0, resid=None, red_y=None, expect=0):
        lib = L.load()
        gin, gchk = guarded((self.M, self.Ci), torch.bfloat16)
        wpart, wchk = guarded((nparts, self.Co, self.Ci), torch.float32)
        redp, rchk = guarded((2, self.Ci, nparts), torch.float32) if red else (None, None)
        c = L.MnasPwBwd()
        c.M, c.Ci, c.Co, c.nparts = self.M, self.Ci, self.Co, nparts
        c.x = act_in(self.x, self.bx[0], self.bx[1]) if self.virt else act_in(self.x)
        c.dy = grad_in(self.g, None if recomp is not None else self.y, self.b)
        c.w, c.gin, c.wpartial = L.ptr(self.wd), L.ptr(gin), L.ptr(wpart)
        c.resid = L.ptr(resid)
        if red:
            c.red_partial, c.red_y, c.red_bn = L.ptr(redp), L.ptr(self.x if red_y is None else red_y), L.ptr(self.bx)
        if recomp is not None:
            c.w_fwd, c.b_fwd = L.ptr(recomp[0]), L.ptr(recomp[1])
        c.gin_masked, c.seg_px = masked, seg_px
        rc = lib.mnas_pw_bwd(C.byref(c), L.cur_stream())
        if expect:
            assert rc == expect, rc
            return None
        L.check(rc, "pw_bwd")
        what = "pw_bwd %dx%d->%d nparts %d%s%s%s" % (self.M, self.Ci, self.Co, nparts, " recomp" if recomp is not None else "",
                                                     " masked" if masked else "", " seg_px %d" % seg_px if seg_px else "")
        gchk(what + " gin")
        wchk(what + " wpartial")
        if red:
            rchk(what + " red_partial")
        return gin, wpart, redp, what

    def check_ref(self, gin, wpart, redp, what, masked=False):
        lib = L.load()
        dy = self.dy()
        ref_gin = dy @ self.w.double()
        if masked:
            ref_gin = ref_gin * _mask(self.x, self.bx[0], self.bx[1])
        assert relerr(gin.double(), ref_gin) < TOL_BF16, (what, "gin", relerr(gin.double(), ref_gin))
        grad, chk = guarded((self.Co, self.Ci), torch.float32)
        # (on a copy: past 256 rows the finalize folds each 128-row chunk into its first row, in place)
        L.check(lib.mnas_wgrad_finalize(L.ptr(wpart.clone()), wpart.shape[0], self.Co, self.Ci, 1, L.ptr(grad), 0, L.cur_stream()))
        chk(what + " dW")
        ref_dw = dy.t() @ self.act()
        assert relerr(grad.double(), ref_dw) < TOL_F32, (what, "dW", relerr(grad.double(), ref_dw))
        if redp is not None:
            # the reduce's dz = gin*[s*x+t>0]: the same sums from a masked gin
            _check_red(redp, gin.float(), self.x.float(), self.bx, what)
            check_red_bound(redp, gin.float(), self.x.float(), self.bx, self.M, what, "fused 1x1 backward: reduce")
        self.check_bounds(gin, grad, wpart.shape[0], what, masked)

    def check_bounds(self, gin, grad, nparts, what, masked):
        """check_onload_bound on gin (dy-on-load interval, rounded to bf16 as pack8 of dy8 stages it; masked: reference, slack and S
        times the mask -- the kernel stores an exact zero there) and check_sum_bound (c = 1) on dW over the act-on-load and
        dy-on-load intervals, pixel chunk by pixel chunk"""
        w64 = self.w.double()
        aw = w64.abs()
        acc = [torch.zeros(self.Co, self.Ci, dtype=torch.float64, device="cuda") for _ in range(3)]
        step = max(1, BOUND_ELEMS // max(self.Ci, self.Co))
        for m0 in range(0, self.M, step):
            m1 = min(self.M, m0 + step)
            d = dy_interval(self.g[m0:m1], self.y[m0:m1], self.b, True, "cuda")
            ref, slack, S = d.mid @ w64, d.half @ aw, d.amax @ aw
            if masked:
                m = relu_mask(self.x[m0:m1], self.bx[0], self.bx[1])
                ref, slack, S = ref * m, slack * m, S * m
            check_onload_bound(gin[m0:m1], ref, slack, S, self.Co, "%s gin pixels %d..%d" % (what, m0, m1), "fused 1x1 backward: gin")
            a = act_interval(self.x[m0:m1], self.bx[0], self.bx[1], True, "cuda") if self.virt else Interval.exact(self.x[m0:m1], "cuda")
            acc[0] += d.mid.t() @ a.mid
            acc[1] += d.amax.t() @ a.amax
            acc[2] += d.mid.abs().t() @ a.mid.abs()
        # slack = sum prod_slack = S - sum |d.mid||a.mid| (amax = |mid| + half)
        check_sum_bound(grad, acc[0], acc[1], self.M, nparts, 1, what + " dW", (acc[1] - acc[2]).clamp_min(0), "fused 1x1 backward: dW")


def _pw_shapes(bit):
    lib = L.load()
    return [s for s in PWB if lib.mnas_pw_bwd_forms(s[3], s[4]) & bit]


def _ids(shapes):
    return ["%dx%dx%d_%d_%d" % s for s in shapes]


RECOMP_PAIRS = [(2, 13, 12, 16, 48), (2, 9, 9, 24, 72), (4, 23, 17, 16, 48)]
MASKED_PAIRS = [s for s in PWB if s[3] > s[4]] + [(3, 37, 29, 48, 16), (2, 31, 29, 72, 24)]


@pytest.mark.parametrize("shape", RECOMP_PAIRS, ids=_ids(RECOMP_PAIRS))
@pytest.mark.parametrize("virt", [True, False], ids=["virt", "plain"])
def test_pw_bwd_recomp(shape, virt):
    """RECOMP (expand convs): y recomputed from the staged x tile must give the stored-y form's results bit for bit"""
    lib = L.load()
    N, H, W, Ci, Co = shape
    assert lib.mnas_pw_bwd_forms(Ci, Co) & 2
    M = N * H * W
    gen = torch.Generator(device="cuda").manual_seed(11)
    cs = _PwCase(M, Ci, Co, gen, virt=virt, bias=True)
    wf = pack(cs.w.view(Co, Ci, 1, 1), L.PACK_FWD)
    # the stored y exactly as the forward writes it
    y, _ = conv_gemm(0, N, H, W, Ci, H, W, Co, 1, 1, 0, wf, cs.bias,
                     act=act_in(cs.x, cs.bx[0], cs.bx[1]) if virt else act_in(cs.x),
                     nparts=max(1, lib.mnas_conv_gemm_parts(0, M, Ci, Co, 1)))
    cs.set_y(y.view(M, Co))
    for nparts in (5, 64):
        a = cs.launch(nparts, red=virt)
        b = cs.launch(nparts, red=virt, recomp=(wf, cs.bias))
        bits_equal(b[0], a[0], a[3] + ": RECOMP vs stored-y gin")
        bits_equal(b[1], a[1], a[3] + ": RECOMP vs stored-y wpartial")
        if virt:
            bits_equal(b[2], a[2], a[3] + ": RECOMP vs stored-y red_partial")
        cs.check_ref(*b)
    # without the forward bias the recomputed y differs: RECOMP must not ignore b_fwd
    if cs.bias is not None:
        c = cs.launch(5, red=virt, recomp=(wf, torch.zeros_like(cs.bias)))
        a = cs.launch(5, red=virt)
        assert not torch.equal(c[1], a[1]), "RECOMP gives the same weight gradient with and without b_fwd"
    # RECOMP exists only where mnas_pw_bwd_forms says so
    other = [s for s in PWB if not lib.mnas_pw_bwd_forms(s[3], s[4]) & 2][0]
    M2 = other[0] * other[1] * other[2]
    co = _PwCase(M2, other[3], other[4], gen, virt=True)
    co.launch(4, recomp=(pack(co.w.view(other[4], other[3], 1, 1), L.PACK_FWD), None), expect=L.EINVAL)


@pytest.mark.parametrize("shape", MASKED_PAIRS, ids=_ids(MASKED_PAIRS))
def test_pw_bwd_gin_masked(shape):
    """gin_masked (project convs feeding a fused depthwise backward): gin stored as gin*[s*x+t>0] under red_bn, bit for bit the
    plain form's gin times the mask (+0 and -0 equal); the reduce and the weight-gradient partials unchanged"""
    lib = L.load()
    N, H, W, Ci, Co = shape
    forms = lib.mnas_pw_bwd_forms(Ci, Co)
    M = N * H * W
    gen = torch.Generator(device="cuda").manual_seed(13)
    cs = _PwCase(M, Ci, Co, gen, virt=True)
    if not forms & 4:
        cs.launch(3, masked=1, expect=L.EINVAL)
        return
    for nparts in (3, 37):
        a = cs.launch(nparts)
        b = cs.launch(nparts, masked=1)
        m = _mask(cs.x, cs.bx[0], cs.bx[1])
        want = torch.where(m, a[0], torch.zeros_like(a[0]))
        bits_equal(b[0], want, b[3] + ": masked gin vs plain gin x mask", signed_zero=False)
        bits_equal(b[2], a[2], b[3] + ": red_partial masked vs plain")
        bits_equal(b[1], a[1], b[3] + ": wpartial masked vs plain")
        cs.check_ref(*b, masked=True)
    # the contract's refusals (csrc/mnas_pwbwd.hip: out-stage form with the fused reduce against x itself only)
    cs.launch(3, red=False, masked=1, expect=L.EINVAL)
    cs.launch(3, masked=1, resid=cs.x, expect=L.EINVAL)
    cs.launch(3, masked=1, red_y=cs.x.clone(), expect=L.EINVAL)


SEG_PAIRS = PWB + [(3, 37, 29, 48, 16), (2, 31, 29, 72, 24)]


@pytest.mark.parametrize("shape", SEG_PAIRS, ids=_ids(SEG_PAIRS))
def test_pw_bwd_segments(shape):
    """segment mode without squeeze-excite: workgroup b owns pixels [b*seg_px, (b+1)*seg_px), last segment ragged; gin bit-identical
    to the strided form, the wpartial rows sum to the same dW"""
    lib = L.load()
    N, H, W, Ci, Co = shape
    M = N * H * W
    tile = lib.mnas_pw_bwd_tile_pixels(Ci, Co)
    assert tile in (64, 128)
    gen = torch.Generator(device="cuda").manual_seed(17)
    cs = _PwCase(M, Ci, Co, gen, virt=True)
    base = cs.launch(7)
    for seg in (tile, tile // 2 + 24, 2 * tile):
        nparts = _cdiv(M, seg)
        assert M % seg != 0 and nparts * seg >= M > (nparts - 1) * seg, (M, seg)
        s = cs.launch(nparts, seg_px=seg)
        bits_equal(s[0], base[0], s[3] + ": gin segment vs strided")
        cs.check_ref(*s)
        cs.launch(nparts - 1, seg_px=seg, expect=L.EINVAL)       # segments do not cover M
        cs.launch(nparts + 1, seg_px=seg, expect=L.EINVAL)       # a segment past the end


# =====================================================================================================================================
# 1.5  mnas_dw_bwd phase 0 on a masked gradient
# =====================================================================================================================================
def _dw_launch(N, H, W, C_, k, nparts, x, bx, g, y, b, wp, phase=0, g_masked=0, red=True, expect=0):
    lib = L.load()
    rows = lib.mnas_dw_rows(N, H, W, C_, k, nparts, 1 if phase == 0 else 3)
    rrows = rows if phase == 0 else lib.mnas_dw_rows(N, H, W, C_, k, nparts, 2)
    assert rows >= 1 and rrows >= 1
    gin, gchk = guarded((N, H, W, C_), torch.bfloat16)
    wpart, wchk = guarded((rows, k * k, C_), torch.float32)
    redp, rchk = guarded((2, C_, rrows), torch.float32) if red else (None, None)
    d = L.MnasDwBwd()
    d.N, d.H, d.W, d.C, d.k, d.nparts = N, H, W, C_, k, nparts
    d.x, d.dy = act_in(x, bx[0], bx[1]), grad_in(g, y, b)
    d.w, d.gin, d.wpartial = L.ptr(wp), L.ptr(gin), L.ptr(wpart)
    if red:
        d.red_bn, d.red_partial = L.ptr(bx), L.ptr(redp)
    d.phase, d.g_masked = phase, g_masked
    rc = lib.mnas_dw_bwd(C.byref(d), L.cur_stream())
    if expect:
        assert rc == expect, rc
        return None
    L.check(rc, "dw_bwd")
    what = "dw_bwd %s k%d nparts %d phase %d%s" % ((N, H, W, C_), k, nparts, phase, " g_masked" if g_masked else "")
    gchk(what + " gin")
    wchk(what + " wpartial")
    if red:
        rchk(what + " red_partial")
    return gin, wpart, redp, rows, what


class _DwCase:
    def __init__(self, N, H, W, C_, k, gen):
        dev = "cuda"
        u = lambda *s: torch.rand(*s, generator=gen, device=dev) * 2 - 1
        self.N, self.H, self.W, self.C, self.k = N, H, W, C_, k
        self.bx = torch.zeros(8, C_, device=dev)
        self.bx[0], self.bx[1] = 1 + 0.3 * u(C_), 0.2 * u(C_)
        self.bx[5], self.bx[6] = 0.1 * u(C_), 1 + 0.2 * u(C_).abs()
        self.b = torch.zeros(8, C_, device=dev)
        self.b[0], self.b[1] = 1 + 0.3 * u(C_), 0.2 * u(C_)
        self.b[2], self.b[3], self.b[4] = self.b[0], 0.05 * u(C_), 0.02 * u(C_)
        self.x = _off_hinge(bf16r(u(N, H, W, C_)), self.bx[0], self.bx[1]).to(torch.bfloat16)     # (the fused reduce's mask input)
        self.g = bf16r(u(N, H, W, C_)).to(torch.bfloat16)
        self.y = _off_hinge(bf16r(u(N, H, W, C_)), self.b[0], self.b[1]).to(torch.bfloat16)
        self.w = u(C_, k, k) * (1.0 / k)
        self.wp = pack(self.w.view(C_, 1, k, k), L.PACK_DW)
        self.gm = torch.where(_mask(self.y, self.b[0], self.b[1]), self.g, torch.zeros_like(self.g))

    def run(self, nparts, masked, **kw):
        g = self.gm if masked else self.g
        return _dw_launch(self.N, self.H, self.W, self.C, self.k, nparts, self.x, self.bx, g, self.y, self.b, self.wp,
                          g_masked=1 if masked else 0, **kw)

    def check_ref(self, r):
        gin, wpart, redp, rows, what = r
        lib = L.load()
        dy = ref_dy(self.g, self.y, self.b, device="cuda")
        ref_gin = ref_dw_dgrad(dy, self.w, device="cuda")
        assert relerr(gin.double(), ref_gin) < TOL_BF16, (what, "gin", relerr(gin.double(), ref_gin))
        a = torch.relu(self.bx[0] * self.x.float() + self.bx[1])
        ref_w = ref_dw_wgrad(a, dy, self.k, device="cuda")
        grad, chk = guarded((self.C, self.k * self.k), torch.float32)
        L.check(lib.mnas_dw_wgrad_finalize(L.ptr(wpart.clone()), rows, self.C, self.k, L.ptr(grad), 0, L.cur_stream()))   # (in place past 256 rows)
        chk(what + " dW")
        assert relerr(grad.double(), ref_w.view(self.C, -1)) < TOL_F32, (what, "dW")
        if redp is not None:
            _check_red(redp, gin.float(), self.x.float(), self.bx, what)
            check_red_bound(redp, gin.float(), self.x.float(), self.bx, self.N * self.H * self.W, what, "fused reduce (depthwise)")
        self.check_bounds(gin, grad.view(self.C, self.k, self.k), rows, what)

    def check_bounds(self, gin, grad, rows, what):
        """check_dw_bound on gin and check_sum_bound (c = 2) on dW over the fp32 intervals of dy and act(x), image chunk by image chunk
        (the weights are fp32 as given; a masked g gives the same dy: dy_interval masks the raw g)"""
        acc = [torch.zeros(self.C, self.k, self.k, dtype=torch.float64, device="cuda") for _ in range(3)]
        step = max(1, BOUND_ELEMS // (self.H * self.W * self.C))
        for n0 in range(0, self.N, step):
            n1 = min(self.N, n0 + step)
            d = dy_interval(self.g[n0:n1], self.y[n0:n1], self.b, False, "cuda")
            ref, S = dw_dgrad_terms(d, self.w, self.H, self.W, 1, "cuda")
            check_dw_bound(gin[n0:n1], ref, S, self.k, "%s gin images %d..%d" % (what, n0, n1), "depthwise input gradient")
            del ref, S
            a = act_interval(self.x[n0:n1], self.bx[0], self.bx[1], False, "cuda")
            for t, v in zip(acc, dw_wgrad_terms(a, d, self.k, 1, "cuda")):
                t += v
        check_sum_bound(grad, acc[0], acc[1], self.N * self.H * self.W, rows, 2, what + " dW", acc[2], "depthwise weight gradient")


@pytest.mark.parametrize("shape", DW, ids=["%dx%dx%dx%d_k%d" % s for s in DW])
def test_dw_bwd_g_masked(shape):
    """g_masked = 1 on bf16(g*mask) against g_masked = 0 on raw g: gin, wpartial and red_partial bit-identical (include/mnas.h)"""
    N, H, W, C_, k = shape
    cs = _DwCase(N, H, W, C_, k, torch.Generator(device="cuda").manual_seed(19))
    for nparts in (37, 1024):
        plain = cs.run(nparts, False)
        m = cs.run(nparts, True)
        bits_equal(m[0], plain[0], m[4] + ": gin")
        bits_equal(m[1], plain[1], m[4] + ": wpartial")
        bits_equal(m[2], plain[2], m[4] + ": red_partial")
        cs.check_ref(m)
    cs.run(37, True, red=False, expect=L.EINVAL)
    cs.run(37, True, phase=1, expect=L.EINVAL)
    cs.run(37, True, phase=2, red=False, expect=L.EINVAL)


# =====================================================================================================================================
# 2.  the launches of the bench configuration's training step, replayed standalone with the production integers
# =====================================================================================================================================
_CENSUS_OPS = {L.OP_PW_BWD: "pw_bwd", L.OP_DW_BWD: "dw_bwd", L.OP_TCONV_DGRAD: "tconv_dgrad", L.OP_DY_MAT: "dy_mat"}
_FORM_SLOTS = {   # pointer slots (by their names in _lib.OP_SLOTS) whose presence selects a form
    L.OP_PW_BWD: {"virt": "x.scale", "red": "red_partial", "resid": "resid", "w_fwd": "w_fwd", "dy.y": "dy.y", "b_fwd": "b_fwd"},
    L.OP_DW_BWD: {"virt": "x.scale", "red": "red_partial", "gin": "gin", "wpartial": "wpartial", "dy.y": "dy.y"},
    L.OP_TCONV_DGRAD: {"red": "stats"}, L.OP_DY_MAT: {"dy.y": "dy.y"},
}


def _census(prog):
    lists = [(prog.fwd_ops, prog.fwd_n)] + [(arr, n) for _, arr, n in prog.bwd_segments]
    seen = {}
    for arr, n in lists:
        for j in range(n):
            o = arr[j]
            if o.opcode not in _CENSUS_OPS:
                continue
            ints = L.op_ints(o)
            if o.opcode == L.OP_DY_MAT:
                ints = ints + (int(L.op_field(o, "rows")),)
            flags = {k: bool(L.op_field(o, s)) for k, s in _FORM_SLOTS[o.opcode].items()}
            key = (o.opcode, ints, tuple(sorted(flags.items())))
            seen[key] = seen.get(key, 0) + 1
    return seen


def _rand(gen, *shape):
    return torch.rand(*shape, generator=gen, device="cuda") * 2 - 1


def _replay_pw(ints, flags, gen, N):
    M, Ci, Co, nparts, masked, seg = ints
    lib = L.load()
    cs = _PwCase(M, Ci, Co, gen, virt=flags["virt"], bias=flags["b_fwd"])
    recomp = None
    if flags["w_fwd"]:
        assert not flags["dy.y"]
        wf = pack(cs.w.view(Co, Ci, 1, 1), L.PACK_FWD)
        # y as the forward stores it (the program's own forward nparts do not change a 1x1 output's bits)
        nfp = lib.mnas_conv_gemm_parts(0, M, Ci, Co, 1)
        nfp = nfp if nfp > 0 else _cdiv(M, lib.mnas_conv_gemm_tile_pixels(M, Co, Ci))
        H = int(round((M // N) ** 0.5))
        assert N * H * H == M
        y, _ = conv_gemm(0, N, H, H, Ci, H, H, Co, 1, 1, 0, wf, cs.bias,
                         act=act_in(cs.x, cs.bx[0], cs.bx[1]) if cs.virt else act_in(cs.x), nparts=nfp)
        cs.set_y(y.view(M, Co))
        recomp = (wf, cs.bias)
    r = cs.launch(nparts, red=flags["red"], recomp=recomp, masked=masked, seg_px=seg)
    cs.check_ref(*r, masked=bool(masked))
    # a second grid: the strided form on another nparts must give the same input gradient bit for bit
    alt = max(1, nparts // 2 + 3)
    r2 = cs.launch(alt, red=flags["red"], recomp=recomp, masked=masked)
    bits_equal(r2[0], r[0], r[3] + ": gin vs nparts %d (strided)" % alt)
    if recomp is not None:
        r3 = cs.launch(nparts, red=flags["red"], masked=masked, seg_px=seg)
        bits_equal(r3[0], r[0], r[3] + ": gin RECOMP vs stored y")
        bits_equal(r3[1], r[1], r[3] + ": wpartial RECOMP vs stored y")
    if masked:
        r4 = cs.launch(nparts, red=True, masked=0, seg_px=seg)
        want = torch.where(_mask(cs.x, cs.bx[0], cs.bx[1]), r4[0], torch.zeros_like(r4[0]))
        bits_equal(r[0], want, r[3] + ": masked gin vs plain x mask", signed_zero=False)
    return "nparts %d / %d" % (nparts, alt)


def _replay_dw(ints, flags, gen, N):
    N, H, W, C_, k, nparts, phase, stride, gm = ints
    assert stride in (0, 1) and phase == 0, "replay covers the fused stride-1 sweep (the only form this config launches)"
    assert flags["red"] or not gm
    cs = _DwCase(N, H, W, C_, k, gen)
    r = cs.run(nparts, bool(gm), red=flags["red"])
    cs.check_ref(r)
    alt = max(1, nparts // 2 + 1)
    r2 = cs.run(alt, bool(gm), red=flags["red"])
    bits_equal(r2[0], r[0], r[4] + ": gin vs nparts %d" % alt)
    if gm:
        r3 = cs.run(nparts, False, red=True)
        bits_equal(r3[0], r[0], r[4] + ": gin g_masked vs raw g")
        bits_equal(r3[1], r[1], r[4] + ": wpartial g_masked vs raw g")
        bits_equal(r3[2], r[2], r[4] + ": red_partial g_masked vs raw g")
    return "nparts %d (%d rows) / %d" % (nparts, r[3], alt)


def _replay_tconv(ints, flags, gen, N):
    N, Ho, Wo, Co, Ci, nparts = ints
    lib = L.load()
    assert nparts == lib.mnas_tconv_parts(N, Ho, Wo, Co, Ci)
    dy = bf16r(_rand(gen, N, Ho, Wo, Co))
    w = bf16r(_rand(gen, Co, Ci, 3, 3) * (1.0 / (9 * Co)) ** 0.5)
    dyd, wp = dy.to(torch.bfloat16), pack(w, L.PACK_TCONV)
    red = None
    if flags["red"]:
        bn = torch.zeros(8, Ci, device="cuda")
        bn[0], bn[1], bn[5], bn[6] = 1 + 0.3 * _rand(gen, Ci), 0.2 * _rand(gen, Ci), 0.1 * _rand(gen, Ci), 1 + 0.2 * _rand(gen, Ci).abs()
        red = (bf16r(_rand(gen, N, 2 * Ho, 2 * Wo, Ci)).to(torch.bfloat16), bn)
    out, st = _tconv_launch(lib, N, Ho, Wo, Co, Ci, dyd, wp, nparts, red)
    ref = ref_dense_dgrad(dy, w, 2 * Ho, 2 * Wo, stride=2, pad=1, device="cuda")
    assert relerr(out.double(), ref) < TOL_BF16, ("tconv", ints, relerr(out.double(), ref))
    del ref
    if red is not None:
        _check_red(st, out.float(), red[0].float(), red[1], "tconv %s" % (ints,))
    alt = nparts + 7 if nparts < 64 else nparts // 2 + 1
    out2, _ = _tconv_launch(lib, N, Ho, Wo, Co, Ci, dyd, wp, alt, red)
    bits_equal(out2, out, "tconv %s: out vs nparts %d" % (ints, alt))
    return "nparts %d / %d" % (nparts, alt)


def _replay_dy_mat(ints, flags, gen, N):
    C_, rows = ints
    lib = L.load()
    g, y = bf16r(_rand(gen, rows, C_)).to(torch.bfloat16), bf16r(_rand(gen, rows, C_)).to(torch.bfloat16)
    b = torch.zeros(8, C_, device="cuda")
    b[0], b[1], b[2], b[3], b[4] = 1 + 0.3 * _rand(gen, C_), 0.2 * _rand(gen, C_), 0, 0.05 * _rand(gen, C_), 0.02 * _rand(gen, C_)
    b[2] = b[0]
    out, chk = guarded((rows, C_), torch.bfloat16)
    gi = grad_in(g, y, b)
    L.check(lib.mnas_dy_materialize(C.byref(gi), rows, C_, L.ptr(out), L.cur_stream()), "dy_materialize")
    chk("dy_materialize %s" % (ints,))
    _check_dy_mat(out, g, y, b, "dy_materialize %s" % (ints,))
    return ""


def test_bench_config_backward_launches():
    """BASELINE configs[1] as bench.py runs it (ccf=False, head '512', bs 256, 224x224, training, default Engine switches): the
    distinct backward launches of the Trainer's Program, each replayed on its own with the production integers (N, shape, nparts,
    phase, flags, seg_px) on device-generated inputs, against fp64 references on the device and bit-identical to a second grid.

    Expected from the engine code (launch_plan.py LaunchPlan._conv_bwd) and asserted: RECOMP (16->48 at 112^2, 24->72 at 56^2), gin_masked
    + segment mode (48->16, 72->24: the project convs in front of fused depthwise sweeps at >= 800 k pixels), gin_masked without
    segments (240->40 at 28^2), g_masked fused depthwise sweeps with k = 3 and k = 5, k_tcx shapes (16->24 at 112^2, 24->40 at
    56^2: the 2x2-block GEMM over dy 56^2 / 28^2), k_tcr (96->192 at 14^2: dy 7x7x192), dy materialised for every dense 3x3."""
    import contextlib
    import io
    from mnasnet_pytorch_amd import FineTuneModelPool, load_model
    from mnasnet_pytorch_amd.train_step import Trainer
    N, HW = 256, 224
    with contextlib.redirect_stdout(io.StringIO()):
        base = load_model("mnasnet")
    m = FineTuneModelPool(base, "mnasnet", 1000, "512").cuda().train()
    tr = Trainer(m, lr=1e-3)
    eng = tr.engine
    eng.ensure_setup(torch.device("cuda"))
    eng._check_modes()
    prog = eng.program(N, HW, HW, True, False, True, False)       # what Trainer.step builds for this batch
    seen = _census(prog)
    prog_gb = torch.cuda.max_memory_allocated() / 2 ** 30
    del prog
    eng.reset_programs()
    del tr, eng, m, base
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()

    keys = sorted(seen, key=lambda k: (k[0], k[1]))
    pw = [(k[1], dict(k[2])) for k in keys if k[0] == L.OP_PW_BWD]
    dw = [(k[1], dict(k[2])) for k in keys if k[0] == L.OP_DW_BWD]
    tc = [(k[1], dict(k[2])) for k in keys if k[0] == L.OP_TCONV_DGRAD]
    dm = [(k[1], dict(k[2])) for k in keys if k[0] == L.OP_DY_MAT]
    # ---- the forms the engine code says this configuration launches
    lib = L.load()
    assert any(f["w_fwd"] and not f["dy.y"] for _, f in pw), "no RECOMP launch"
    assert {(i[1], i[2]) for i, f in pw if f["w_fwd"]} >= {(16, 48), (24, 72)}
    assert any(i[4] for i, _ in pw), "no gin_masked launch"
    assert {(i[1], i[2]) for i, _ in pw if i[5] > 0} >= {(48, 16), (72, 24)}, "segment mode missing on the 112^2 / 56^2 project convs"
    assert all(i[3] * i[5] >= i[0] > (i[3] - 1) * i[5] for i, _ in pw if i[5] > 0)
    assert {i[4] for i, _ in dw if i[8]} >= {3, 5}, "g_masked fused depthwise sweeps of both kernel sizes"
    assert all(i[6] == 0 for i, _ in dw), "dw_fused_k = (3, 5): every stride-1 depthwise backward is one fused sweep"
    assert {(i[1], i[3], i[4]) for i, _ in tc} >= {(56, 24, 16), (28, 40, 24), (7, 192, 96)}, "k_tcx / k_tcr shapes"
    assert all(lib.mnas_tconv_parts(*i[:5]) == i[5] for i, _ in tc)
    assert all(f["dy.y"] for _, f in dm)
    assert all((i[3], i[0] * i[1] * i[2]) in {(d[0], d[1]) for d, _ in dm} for i, _ in tc), "a tconv launch without its dy_mat"
    # ---- census: forms x shapes x nparts
    lines = []
    gen = torch.Generator(device="cuda").manual_seed(2026)
    replay = {L.OP_PW_BWD: _replay_pw, L.OP_DW_BWD: _replay_dw, L.OP_TCONV_DGRAD: _replay_tconv, L.OP_DY_MAT: _replay_dy_mat}
    for k in keys:
        opc, ints, flags = k[0], k[1], dict(k[2])
        form = _CENSUS_OPS[opc]
        if opc == L.OP_PW_BWD:
            form += "".join([" RECOMP" if flags["w_fwd"] else "", " gin_masked" if ints[4] else "", " seg_px=%d" % ints[5] if ints[5] else "",
                             " red" if flags["red"] else "", " resid" if flags["resid"] else "", " virt" if flags["virt"] else ""])
        elif opc == L.OP_DW_BWD:
            form += " k%d phase %d%s%s" % (ints[4], ints[6], " g_masked" if ints[8] else "", " red" if flags["red"] else "")
        elif opc == L.OP_TCONV_DGRAD:
            form += (" k_tcr" if ints[3] == 192 else " k_tcx" if lib.mnas_tconv_parts(*ints[:5]) <= 1024 and ints[3] <= 40 else " k_tconv") + \
                (" red" if flags["red"] else "")
        torch.cuda.synchronize()
        what = replay[opc](ints, flags, gen, N)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        lines.append("%-52s ints %-44s x%d  %s" % (form, ints, seen[k], what))
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print("\nbench-config backward census (%d distinct launches; Program build peak %.1f GB, replay peak %.1f GB):\n  %s"
          % (len(keys), prog_gb, peak, "\n  ".join(lines)))
    assert peak < 20
