"""-m gpu: the forward, weight-gradient and stem launches in the forms and at the gates the training step runs them.

Part 1 (small and medium shapes): the kernel family mnas_conv_gemm's dispatcher picks for every shape of test_gpu_kernels.PW /
DENSE and for both sides of each numeric gate (asserted through mnas_conv_gemm_route, which shares the dispatcher with the launch);
every k_igemm (MODE, NT, PT) instance; the stem's fused input pipeline (uint8 / float image, in_affine) against a host-built table
of the 768 staged values, bit for bit; the plain-input depthwise forward; M = 2^24 pixels, where the pixel decode switches from
the reciprocal to exact division.  Part 2: the distinct forward / weight-gradient / stem / glue launches of the bench
configuration's two training Programs (float and uint8 input), replayed standalone with the production integers.

Every output, statistics table and partial slab lives in a guarded buffer (tests/gpu_util.py).  References are fp64, built from
slicing and matmul (refs64.ref_*), on the device.  Launches whose operand needs no transform on load are held to the
per-element bound of bounds_conv.check_gemm_bound; those with act-on-load / dy-on-load to bounds_conv.check_onload_bound over the
operand's interval (the same bound plus the interval's slack), their statistics to check_stats_bound, their fused reduce to
check_red_bound; the depthwise forward with fp32 weights to check_dw_bound.  The max-normalised tolerances are asserted as well."""
import ctypes as C
from fractions import Fraction

import pytest
import torch

from bounds_conv import (act_interval, check_dw_bound, check_gemm_bound, check_onload_bound, check_red_bound, dw_elem_err, dw_fwd_terms,
                         dy_interval, onload_dgrad_terms, onload_elem_err, onload_fwd_terms, stats_bound_terms)
from gpu_util import L, act_in, bf16r, bits_equal, conv_gemm, grad_in, guarded, pack, relerr, route_of
from intervals import Interval, check_sum_bound
from refs64 import ref_dense_dgrad, ref_dense_fwd, ref_dense_wgrad, ref_dw_fwd, ref_dy, ref_stem, ref_stem_wgrad
from test_gpu_bwd_forms import _cdiv, _check_red, _off_hinge, _rand
from test_gpu_kernels import DENSE, DW, PW, TOL_BF16, TOL_F32

pytestmark = pytest.mark.gpu
CHUNK_ELEMS = 48 << 20          # fp64 elements of the largest tensor of one reference chunk (images are never cut)


def _bn(gen, C_):
    b = torch.zeros(8, C_, device="cuda")
    b[0], b[1] = 1 + 0.3 * _rand(gen, C_), 0.2 * _rand(gen, C_)
    b[2], b[3], b[4] = b[0], 0.05 * _rand(gen, C_), 0.02 * _rand(gen, C_)
    b[5], b[6] = 0.1 * _rand(gen, C_), 1 + 0.2 * _rand(gen, C_).abs()
    return b


def _img_chunks(N, per_image):
    step = max(1, min(N, CHUNK_ELEMS // max(1, per_image)))
    return [(n0, min(N, n0 + step)) for n0 in range(0, N, step)]


# =====================================================================================================================================
# one mnas_conv_gemm problem: the conv (N,H,W,Ci) -> (N,Ho,Wo,Co), k x k, pad k//2; mode 0 runs it forward, mode 1 its input gradient
# =====================================================================================================================================
class _GemmCase:
    """Device operands of one launch, seeded by `gen`.  mode 0: x read plain or through (scale, shift) (virt), bias.  mode 1: dy
    as dy-on-load of (g, y, coef) or materialised (coef=False: g IS dy), optional residual, optional fused BatchNorm-backward
    reduce against (y_in, b_in) with y_in moved off the ReLU hinge."""
    def __init__(self, mode, N, H, W, Ci, Co, k, stride, gen, virt=True, coef=True, resid=False, red=False, bias=True):
        self.mode, self.N, self.H, self.W, self.Ci, self.Co, self.k, self.stride = mode, N, H, W, Ci, Co, k, stride
        self.pad = k // 2
        self.Ho, self.Wo = (H + 2 * self.pad - k) // stride + 1, (W + 2 * self.pad - k) // stride + 1
        self.virt, self.coef = virt, coef
        self.w = bf16r(_rand(gen, Co, Ci, k, k) * (3.0 / (k * k * (Ci if mode == 0 else Co))) ** 0.5)
        self.wp = pack(self.w, L.PACK_FWD if mode == 0 else L.PACK_DGRAD)
        self.bias = self.resid = self.y_in = self.b_in = None
        if mode == 0:
            self.x = bf16r(_rand(gen, N, H, W, Ci)).to(torch.bfloat16)
            self.sc, self.sh = 1 + 0.3 * _rand(gen, Ci), 0.2 * _rand(gen, Ci)
            self.bias = 0.1 * _rand(gen, Co) if bias else None
        else:
            self.g = bf16r(_rand(gen, N, self.Ho, self.Wo, Co)).to(torch.bfloat16)
            self.b = _bn(gen, Co) if coef else None
            self.y = _off_hinge(bf16r(_rand(gen, N, self.Ho, self.Wo, Co)), self.b[0], self.b[1]).to(torch.bfloat16) if coef else None
            if resid:
                self.resid = bf16r(_rand(gen, N, H, W, Ci)).to(torch.bfloat16)
            if red:
                self.b_in = _bn(gen, Ci)
                self.y_in = _off_hinge(bf16r(_rand(gen, N, H, W, Ci)), self.b_in[0], self.b_in[1]).to(torch.bfloat16)

    @property
    def plain(self):
        return (self.mode == 0 and not self.virt) or (self.mode == 1 and not self.coef)

    def route(self):
        if self.mode == 0:
            return route_of(0, self.N, self.H, self.W, self.Ci, self.Ho, self.Wo, self.Co, self.k, self.stride, self.pad,
                            virt=self.virt, bias=self.bias is not None)
        return route_of(1, self.N, self.Ho, self.Wo, self.Co, self.H, self.W, self.Ci, self.k, self.stride, self.pad,
                        coef=self.coef, resid=self.resid is not None)

    def launch(self, nparts, stats=True):
        sink = []
        if self.mode == 0:
            out, st = conv_gemm(0, self.N, self.H, self.W, self.Ci, self.Ho, self.Wo, self.Co, self.k, self.stride, self.pad, self.wp,
                                self.bias, act=act_in(self.x, self.sc if self.virt else None, self.sh if self.virt else None),
                                nparts=nparts, stats=stats, guard=True, route=sink)
        else:
            red = self.y_in is not None
            out, st = conv_gemm(1, self.N, self.Ho, self.Wo, self.Co, self.H, self.W, self.Ci, self.k, self.stride, self.pad, self.wp,
                                None, grad=grad_in(self.g, self.y, self.b), resid=self.resid, nparts=nparts, stats=red,
                                red_y=self.y_in, red_bn=self.b_in, guard=True, route=sink)
        assert sink[0] == self.route(), ("the route of the launched struct differs from the flag-built one", sink[0], self.route())
        return out, st

    def what(self):
        return "conv_gemm mode %d %dx%dx%dx%d -> %d k%d s%d %s%s%s" % (
            self.mode, self.N, self.H, self.W, self.Ci, self.Co, self.k, self.stride,
            ("virt" if self.virt else "plain") if self.mode == 0 else ("dy-on-load" if self.coef else "materialised dy"),
            " resid" if self.resid is not None else "", " red" if self.y_in is not None else "")

    def check(self, out, st, images=None):
        """fp64 on the device, image chunk by image chunk; `images`: a subset (the statistics then are not compared).
        Plain operand: check_gemm_bound.  Operand formed on load: check_onload_bound over act_interval / dy_interval (bf16 ends), the
        reference being the interval's midpoint; forward statistics: check_stats_bound terms summed over the chunks (the epilogues sum
        the fp32 accumulator, whose own error is onload_elem_err); fused reduce: check_red_bound on the output as stored."""
        what = self.what()
        K = self.k * self.k * (self.Ci if self.mode == 0 else self.Co)
        per = max(self.H * self.W * self.Ci, self.Ho * self.Wo * self.Co) * (self.k * self.k if self.k > 1 else 1)
        chunks = _img_chunks(self.N, per) if images is None else [(n, n + 1) for n in images]
        s1 = torch.zeros(self.Co, dtype=torch.float64, device="cuda")
        s2 = torch.zeros_like(s1)
        worst, scale = 0.0, 0.0
        errs = []
        sterms = None
        for n0, n1 in chunks:
            if self.mode == 0:
                iv = act_interval(self.x[n0:n1], self.sc, self.sh, True, "cuda") if self.virt else Interval.exact(self.x[n0:n1], "cuda")
                ref, slack, S = onload_fwd_terms(iv, self.w, self.bias, self.stride, self.pad, "cuda")
                del iv
                s1 += ref.sum((0, 1, 2))
                s2 += (ref * ref).sum((0, 1, 2))
                t = stats_bound_terms(ref, onload_elem_err(slack, S, K))
                sterms = t if sterms is None else tuple(a_ + b_ for a_, b_ in zip(sterms, t))
            else:
                gs = self.g[n0:n1]
                iv = dy_interval(gs, self.y[n0:n1], self.b, True, "cuda") if self.coef else Interval.exact(gs, "cuda")
                ref, slack, S = onload_dgrad_terms(iv, self.w, self.H, self.W, self.stride, self.pad,
                                                   None if self.resid is None else self.resid[n0:n1], "cuda")
                del iv
            if self.plain:
                assert float(slack.max()) == 0.0
                worst = max(worst, check_gemm_bound(out[n0:n1], ref, S, K, "%s images %d..%d" % (what, n0, n1)))
            else:
                worst = max(worst, check_onload_bound(out[n0:n1], ref, slack, S, K, "%s images %d..%d" % (what, n0, n1),
                                                      "%s %s" % ("1x1" if self.k == 1 else "3x3", "forward" if self.mode == 0 else "input gradient")))
            del S, slack
            errs.append(float((out[n0:n1].double() - ref).abs().max()))
            scale = max(scale, float(ref.abs().max()))
            del ref
        rel = max(errs) / (scale + 1e-12)
        assert rel < TOL_BF16, (what, "max-normalised error", rel)
        if images is None and self.mode == 0 and st is not None:
            p = st.double().sum(-1)
            assert relerr(p[0], s1) < TOL_F32, (what, "stats sum", relerr(p[0], s1))
            assert relerr(p[1], s2) < TOL_F32, (what, "stats sum of squares", relerr(p[1], s2))
            Mo, P = self.N * self.Ho * self.Wo, st.shape[-1]
            check_sum_bound(p[0], sterms[0], sterms[1], Mo, P, 1, what + " stats sum", sterms[2], "forward statistics")
            check_sum_bound(p[1], sterms[3], sterms[4], Mo, P, 2, what + " stats sum of squares", sterms[5], "forward statistics")
        if images is None and self.mode == 1 and st is not None:
            _check_red(st, out.float(), self.y_in.float(), self.b_in, what)
            check_red_bound(st, out.float(), self.y_in.float(), self.b_in, self.N * self.H * self.W, what, "fused reduce (GEMM)")
        return rel, worst


def _case_from(spec, gen):
    mode, N, H, W, Ci, Co, k, s, form = spec
    return _GemmCase(mode, N, H, W, Ci, Co, k, s, gen, **form)


def _run_case(cs, expect_route, expect_inst=None, nparts=(13, 38)):
    r, inst = cs.route()
    assert r == expect_route, (cs.what(), "route", r, inst, "expected", expect_route)
    if expect_inst is not None:
        assert inst[:len(expect_inst)] == tuple(expect_inst), (cs.what(), "k_igemm instance", inst, "expected", expect_inst)
    outs = []
    for p in nparts:
        out, st = cs.launch(p)
        cs.check(out, st)
        outs.append(out)
    for o in outs[1:]:
        bits_equal(o, outs[0], cs.what() + ": out vs another grid")


# =====================================================================================================================================
# 1.1  routes
# =====================================================================================================================================
# what the comments of test_gpu_kernels.PW / DENSE claim per entry, corrected where the dispatcher says otherwise (marked !):
#   PW[16] 192 -> 1152 sits under the "csrc/mnas_pwx.hip" comment but k_pwx is not instantiated for Ci > 96: k_pws (K >= 192);
#   DENSE[6], [7] (Ci >= 64 onto a <= 64-pixel plane, 9*Ci*Co >= 128 K) sit under "csrc/mnas_dimg.hip" but k_c3r is tried first;
#   DENSE[8], [10] are stride 2 onto <= 64 pixels, which k_dimg refuses: k_igemm.  No entry of DENSE reaches k_dimg with stride 2
#   (it needs 64 < output plane <= 256); DIMG_S2 below adds that form, which the bench configuration runs (40 -> 80, 28^2 -> 14^2).
PW_FWD_ROUTE = ["k_pwf", "k_igemm", "k_igemm", "k_pwx", "k_pws", "k_igemm", "k_pws", "k_pwx", "k_pws", "k_pws", "k_igemm",
                "k_pwx", "k_pwx", "k_pwx", "k_pwx", "k_pwx", "k_pws", "k_pwf"]          # [16] !
DENSE_FWD_ROUTE = ["k_igemm"] * 5 + ["k_dimg", "k_c3r", "k_c3r", "k_igemm", "k_dimg", "k_igemm"] + ["k_c3r"] * 4 + ["k_c3x"] * 3   # [6] [7] [8] [10] !


def _pw_d_route(Ci, Co, coef, resid):
    """1x1 input gradient (dy has Co channels, the result Ci): k_pws takes dy-on-load with a long reduction (Co >= 192) whose
    result tiles pad by at most three; k_pwd a widening result (Ci > Co, Co <= 128) without a residual; the rest is k_igemm"""
    tiles = (Ci + 15) // 16
    nt = 3 if tiles <= 3 else 6
    ksteps = (Co + 31) // 32
    nw = 8 if (ksteps > 20 or ksteps >= 12) else 4
    if coef and Co >= 192 and _cdiv(tiles, nt) * nt - tiles <= 3 and _cdiv(ksteps, nw) <= 3:
        return "k_pws"
    if not resid and Ci > Co and Co <= 128:
        return "k_pwd"
    return "k_igemm"


def _dense_d_route(N, H, W, Ci, Co, s, coef):
    """3x3 input gradient: the whole-image kernels take a materialised dy at stride 1 and N >= 32 only (k_c3r: result plane <= 64
    pixels, Co >= 64 dy channels, 9*Co*Ci >= 128 K; k_dimg: result plane <= 256 pixels, Co >= 16)"""
    if coef or s != 1 or N < 32:
        return "k_igemm"
    if H * W <= 64 and Co >= 64 and 9 * Ci * Co >= 128 * 1024:
        return "k_c3r"
    return "k_dimg" if H * W <= 256 and Co >= 16 else "k_igemm"


def _list_routes():
    seen = set()
    for j, (N, H, W, Ci, Co) in enumerate(PW):
        for virt in (True, False):
            r = route_of(0, N, H, W, Ci, H, W, Co, 1, 1, 0, virt=virt)
            assert r[0] == PW_FWD_ROUTE[j], ("PW[%d] forward" % j, PW[j], r)
            seen.add((0,) + r)
        for coef, resid in ((True, False), (True, True), (False, False)):
            r = route_of(1, N, H, W, Co, H, W, Ci, 1, 1, 0, coef=coef, resid=resid)
            assert r[0] == _pw_d_route(Ci, Co, coef, resid), ("PW[%d] input gradient coef=%s resid=%s" % (j, coef, resid), PW[j], r)
            seen.add((1,) + r)
    for j, (N, H, W, Ci, Co, s) in enumerate(DENSE):
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        r = route_of(0, N, H, W, Ci, Ho, Wo, Co, 3, s, 1)
        assert r[0] == DENSE_FWD_ROUTE[j], ("DENSE[%d] forward" % j, DENSE[j], r)
        seen.add((0,) + r)
        for coef in (True, False):
            r = route_of(1, N, Ho, Wo, Co, H, W, Ci, 3, s, 1, coef=coef)
            assert r[0] == _dense_d_route(N, H, W, Ci, Co, s, coef), ("DENSE[%d] input gradient coef=%s" % (j, coef), DENSE[j], r)
            if s == 2 and not (H & 1) and not (W & 1):
                assert r[1][3] == 1, ("DENSE[%d]: even plane, stride 2: the parity-class form" % j, r)
            seen.add((1,) + r)
    return seen


V, P = dict(virt=True), dict(virt=False)
DC, DM, DR = dict(coef=True), dict(coef=False), dict(coef=True, resid=True)
# (mode, N, H, W, Ci, Co, k, stride, form), route, k_igemm (NT, PT) or None -- both sides of every numeric gate of the dispatcher
GATES = [
    # k_pwx: M <= 250 000 (a whole number of 16-pixel groups: 15 625); one group more runs on k_pwf
    ((0, 250, 25, 40, 40, 240, 1, 1, V), "k_pwx", None), ((0, 13, 601, 32, 40, 240, 1, 1, V), "k_pwf", None),
    ((0, 250, 25, 40, 40, 240, 1, 1, P), "k_pwx", None), ((0, 13, 601, 32, 40, 240, 1, 1, P), "k_pwf", None),
    # k_pws: M <= 250 000; beyond it the narrowing conv is k_igemm's
    ((0, 250, 25, 40, 240, 40, 1, 1, V), "k_pws", None), ((0, 13, 601, 32, 240, 40, 1, 1, V), "k_igemm", (3, 2)),
    ((0, 250, 25, 40, 240, 40, 1, 1, P), "k_pws", None), ((0, 13, 601, 32, 240, 40, 1, 1, P), "k_igemm", (3, 2)),
    # k_pwf: 64-pixel tiles below M = 400 000, 128-pixel tiles from there
    ((0, 39, 641, 16, 16, 48, 1, 1, V), "k_pwf", None), ((0, 250, 40, 40, 16, 48, 1, 1, V), "k_pwf", None),
    ((0, 39, 641, 16, 16, 48, 1, 1, P), "k_pwf", None), ((0, 250, 40, 40, 16, 48, 1, 1, P), "k_pwf", None),
    # k_igemm: PT = 2 from M * cout blocks = 131 072
    ((0, 8191, 4, 4, 48, 16, 1, 1, V), "k_igemm", (1, 1)), ((0, 32, 64, 64, 48, 16, 1, 1, V), "k_igemm", (1, 2)),
    ((0, 8191, 4, 4, 48, 16, 1, 1, P), "k_igemm", (1, 1)), ((0, 32, 64, 64, 48, 16, 1, 1, P), "k_igemm", (1, 2)),
    # k_dimg: N >= 32
    ((0, 31, 14, 14, 80, 96, 3, 1, V), "k_igemm", (6, 1)), ((0, 32, 14, 14, 80, 96, 3, 1, V), "k_dimg", None),
    ((1, 31, 14, 14, 80, 96, 3, 1, DM), "k_igemm", (6, 1)), ((1, 32, 14, 14, 80, 96, 3, 1, DM), "k_dimg", None),
]
# k_dimg at stride 2 (64 < output plane <= 256 pixels), ragged planes included; no DENSE entry reaches it
DIMG_S2 = [((0, 32, 28, 28, 40, 80, 3, 2, V), "k_dimg", None), ((0, 33, 27, 25, 24, 40, 3, 2, V), "k_dimg", None),
           ((0, 32, 28, 28, 40, 80, 3, 2, P), "k_dimg", None)]
# every k_igemm (MODE, NT, PT) the MNAS_IG table instantiates that the lists above leave out; ragged last tiles; plain operands
# where the per-element bound applies.  k-chunks 32 / 64 / 128 and the parity-class form come from the lists.
IGEMM = [
    ((0, 2, 12, 13, 24, 24, 1, 1, P), "k_igemm", (2, 1)), ((0, 33, 63, 65, 24, 24, 1, 1, P), "k_igemm", (2, 2)),
    ((0, 33, 63, 65, 40, 40, 1, 1, V), "k_igemm", (3, 2)), ((0, 2, 12, 13, 64, 64, 1, 1, P), "k_igemm", (4, 1)),
    ((0, 9, 63, 61, 160, 256, 1, 1, P), "k_igemm", (4, 2)), ((0, 33, 63, 65, 72, 72, 1, 1, P), "k_igemm", (6, 2)),
    ((0, 2, 12, 13, 104, 104, 1, 1, V), "k_igemm", (8, 1)), ((0, 33, 63, 65, 104, 104, 1, 1, P), "k_igemm", (8, 2)),
    ((1, 33, 63, 65, 8, 8, 1, 1, DM), "k_igemm", (1, 2)), ((1, 33, 63, 65, 24, 8, 1, 1, DR), "k_igemm", (2, 2)),
    ((1, 33, 63, 65, 40, 8, 1, 1, DR), "k_igemm", (3, 2)), ((1, 2, 12, 13, 64, 8, 1, 1, DR), "k_igemm", (4, 1)),
    ((1, 9, 63, 61, 256, 8, 1, 1, DR), "k_igemm", (4, 2)), ((1, 33, 63, 65, 72, 8, 1, 1, DR), "k_igemm", (6, 2)),
    ((1, 2, 12, 13, 104, 8, 1, 1, DR), "k_igemm", (8, 1)), ((1, 33, 63, 65, 104, 8, 1, 1, DR), "k_igemm", (8, 2)),
    # the remaining cases of the Ci % 32 != 0 last k-step, 3x3 with a materialised dy and the fused reduce on k_igemm
    ((0, 3, 11, 9, 40, 24, 3, 1, P), "k_igemm", (2, 1)), ((1, 3, 11, 9, 24, 40, 3, 1, DM), "k_igemm", (2, 1)),
    ((1, 3, 12, 10, 24, 40, 3, 2, DM), "k_igemm", (2, 1)),
]
ALL_CASES = GATES + DIMG_S2 + IGEMM


def _cid(c):
    spec = c[0]
    return "m%d_%dx%dx%dx%d_%d_k%ds%d_%s" % (spec[:8] + ("".join(sorted(k for k, v in spec[8].items() if v)) or "plain",))


def test_routes_of_the_existing_lists_and_full_cover():
    """Every entry of PW / DENSE reaches the family the lists' comments name (corrections listed at PW_FWD_ROUTE); the union of the
    routes of those lists and of this file's cases contains every MNAS_ROUTE_* value, every (MODE, NT, PT) instance of the MNAS_IG
    table, k-chunks 32, 64 and 128 and the parity-class form.  No instance of the table is unreachable."""
    seen = _list_routes()
    for spec, route, inst in ALL_CASES:
        mode, N, H, W, Ci, Co, k, s, form = spec
        p = k // 2
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        r = route_of(0, N, H, W, Ci, Ho, Wo, Co, k, s, p, **form) if mode == 0 else route_of(1, N, Ho, Wo, Co, H, W, Ci, k, s, p, **form)
        assert r[0] == route and (inst is None or r[1][:2] == inst), (spec, r, route, inst)
        seen.add((mode,) + r)
    fams = {(m, r) for m, r, _ in seen}
    want = {(0, "k_pwx"), (0, "k_pws"), (1, "k_pws"), (0, "k_pwf"), (1, "k_pwd"), (0, "k_c3r"), (1, "k_c3r"), (0, "k_dimg"), (1, "k_dimg"),
            (0, "k_c3x"), (0, "k_igemm"), (1, "k_igemm")}
    assert fams >= want, ("families without a case", sorted(want - fams))
    ig = {(m, i[0], i[1]) for m, r, i in seen if r == "k_igemm"}
    table = {(m, nt, pt) for m in (0, 1) for nt in (1, 2, 3, 4, 6, 8) for pt in (1, 2)}
    assert ig >= table, ("k_igemm instances without a case", sorted(table - ig))
    assert {i[2] for m, r, i in seen if r == "k_igemm"} == {32, 64, 128}
    assert any(i[3] for m, r, i in seen if r == "k_igemm" and m == 1), "parity-class form"
    # the query refuses what the launch refuses
    assert L.load().mnas_conv_gemm_route(None, None) == -L.EINVAL
    bad = L.MnasConvGemm()
    bad.mode = 2
    assert L.load().mnas_conv_gemm_route(C.byref(bad), None) == -L.EINVAL


@pytest.mark.parametrize("case", ALL_CASES, ids=[_cid(c) for c in ALL_CASES])
def test_gate_sides_and_igemm_instances(case):
    spec, route, inst = case
    gen = torch.Generator(device="cuda").manual_seed(31)
    cs = _case_from(spec, gen)
    M = cs.N * cs.Ho * cs.Wo if cs.mode == 0 else cs.N * cs.H * cs.W
    _run_case(cs, route, inst, nparts=(13, 38) if M < 100000 else (96, 331))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("j", range(len(PW)), ids=["%dx%dx%dx%d_%d" % s for s in PW])
def test_pw_lists_plain_operand_bound(j):
    """PW entries with operands that need no transform on load: the per-element bound, forward and input gradient"""
    N, H, W, Ci, Co = PW[j]
    gen = torch.Generator(device="cuda").manual_seed(37)
    _run_case(_GemmCase(0, N, H, W, Ci, Co, 1, 1, gen, virt=False), PW_FWD_ROUTE[j])
    _run_case(_GemmCase(1, N, H, W, Ci, Co, 1, 1, gen, coef=False), _pw_d_route(Ci, Co, False, False))


@pytest.mark.parametrize("j", range(len(DENSE)), ids=["%dx%dx%dx%d_%d_s%d" % s for s in DENSE])
def test_dense_lists_plain_operand_bound(j):
    N, H, W, Ci, Co, s = DENSE[j]
    gen = torch.Generator(device="cuda").manual_seed(41)
    _run_case(_GemmCase(0, N, H, W, Ci, Co, 3, s, gen, virt=False), DENSE_FWD_ROUTE[j], nparts=(5, 17))
    _run_case(_GemmCase(1, N, H, W, Ci, Co, 3, s, gen, coef=False, red=(s == 1)), _dense_d_route(N, H, W, Ci, Co, s, False), nparts=(5, 17))
    torch.cuda.empty_cache()


# =====================================================================================================================================
# 1.2  stem input forms
# =====================================================================================================================================
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # classifiers.py


def _engine_affine(u8):
    """Engine.input_affine: scale 1/(k*std), shift -mean/std, formed in fp64 and rounded to fp32"""
    m, s = torch.tensor(MEAN, dtype=torch.float64), torch.tensor(STD, dtype=torch.float64)
    return torch.stack([1.0 / ((255.0 if u8 else 1.0) * s), -m / s]).to(torch.float32)


WILD_AFFINE = torch.tensor([[-2.0, 0.3, -0.0117], [300.0, -77.5, 3.0]], dtype=torch.float32)     # negative scales, large shifts


def _staged_table(aff):
    """[3][256] fp32 holding the bf16 value the kernel stages for byte u of plane c: bf16(fmaf(u, scale, shift)).  Proved on the host
    for this very affine: u*scale + shift is exact in fp64 (so its rounding to fp32 IS fmaf) and no value is a bf16 tie."""
    t64 = torch.arange(256, dtype=torch.float64).view(1, 256) * aff[0].double().view(3, 1) + aff[1].double().view(3, 1)
    for c in range(3):
        sc, sh = Fraction(float(aff[0, c])), Fraction(float(aff[1, c]))
        for u in range(256):
            assert Fraction(float(t64[c, u])) == u * sc + sh, ("u*scale+shift not exact in fp64", c, u)
    t32 = t64.to(torch.float32)
    assert not bool(((t32.view(torch.int32) & 0xFFFF) == 0x8000).any()), "a staged value lies on a bf16 tie"
    return bf16r(t32)


def test_staged_table_of_the_engine_affine_is_exact():
    """all 768 (u, c) of the engine's own uint8 affine: fp64 equals the rational result, none on a bf16 tie (host only)"""
    tab = _staged_table(_engine_affine(True))
    assert tab.shape == (3, 256) and bool((tab[:, 1:] >= tab[:, :-1]).all())
    _staged_table(WILD_AFFINE)


def _stem_fwd(x, N, H, W, Co, wp, bias, nparts, aff=None, u8=0, expect=0):
    lib = L.load()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out, ochk = guarded((N, Ho, Wo, Co), torch.bfloat16)
    st, schk = guarded((2, Co, nparts), torch.float32)
    a = L.MnasStemFwd()
    a.N, a.H, a.W, a.Ho, a.Wo, a.Co, a.nparts = N, H, W, Ho, Wo, Co, nparts
    a.x, a.w, a.bias, a.out, a.stats = L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(out), L.ptr(st)
    a.in_affine, a.in_u8 = L.ptr(aff), u8
    rc = lib.mnas_stem_fwd(C.byref(a), L.cur_stream())
    what = "stem_fwd %s nparts %d%s%s" % ((N, H, W, Co), nparts, " u8" if u8 else "", " affine" if aff is not None else "")
    if expect:
        assert rc == expect, (what, rc)
        torch.cuda.synchronize()
        ochk(what + " out (refused)", written=False)
        assert bool((out.view(torch.int16) == 0x7FA5).all()) and bool((st.view(torch.int32) == 0x7FA5A5A5).all()), what + ": a refused launch wrote"
        return None, None
    L.check(rc, what)
    ochk(what + " out")
    schk(what + " stats")
    return out, st


def _stem_wgrad(x, N, H, W, Co, dy, nparts, aff=None, u8=0, expect=0):
    lib = L.load()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    part, pchk = guarded((nparts, Co, 27), torch.float32)
    s = L.MnasStemWgrad()
    s.N, s.H, s.W, s.Ho, s.Wo, s.Co, s.nparts = N, H, W, Ho, Wo, Co, nparts
    s.x, s.dy, s.partial = L.ptr(x), dy, L.ptr(part)
    s.in_affine, s.in_u8 = L.ptr(aff), u8
    rc = lib.mnas_stem_wgrad(C.byref(s), L.cur_stream())
    what = "stem_wgrad %s nparts %d%s%s" % ((N, H, W, Co), nparts, " u8" if u8 else "", " affine" if aff is not None else "")
    if expect:
        assert rc == expect, (what, rc)
        torch.cuda.synchronize()
        assert bool((part.view(torch.int32) == 0x7FA5A5A5).all()), what + ": a refused launch wrote"
        return None
    L.check(rc, what)
    pchk(what + " partial")
    return part


def _stem_finalize(part, Co):
    grad, chk = guarded((Co, 3, 3, 3), torch.float32)
    L.check(L.load().mnas_wgrad_finalize(L.ptr(part.clone()), part.shape[0], Co, 27, 1, L.ptr(grad), 0, L.cur_stream()))
    chk("stem dW")
    return grad


def _stem_check_fp64(t, w, bias, dy64, out, st, part, what):
    """t: (N,3,H,W) fp32 cuda holding the staged bf16 values"""
    ref = ref_stem(t, w, bias, device="cuda")
    assert relerr(out.double(), ref) < TOL_BF16, (what, "out", relerr(out.double(), ref))
    # the border rows / columns on their own: the only pixels that see the zero padding
    for name, sl in (("top row", (slice(None), slice(0, 1))), ("left column", (slice(None), slice(None), slice(0, 1))),
                     ("bottom row", (slice(None), slice(-1, None))), ("right column", (slice(None), slice(None), slice(-1, None)))):
        assert relerr(out[sl].double(), ref[sl]) < TOL_BF16, (what, name, relerr(out[sl].double(), ref[sl]))
    p = st.double().sum(-1)
    assert relerr(p[0], ref.sum((0, 1, 2))) < TOL_F32, (what, "stats sum", relerr(p[0], ref.sum((0, 1, 2))))
    assert relerr(p[1], (ref * ref).sum((0, 1, 2))) < TOL_F32, (what, "stats sum of squares", relerr(p[1], (ref * ref).sum((0, 1, 2))))
    if part is not None:
        grad = _stem_finalize(part, w.shape[0])
        rw = ref_stem_wgrad(t, dy64, device="cuda")
        assert relerr(grad.double(), rw) < TOL_F32, (what, "dW", relerr(grad.double(), rw))
    return ref


STEM_SHAPES = [(2, 12, 12), (3, 40, 48), (2, 37, 32), (11, 18, 16), (2, 224, 224), (1, 34, 80)]


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=["%dx%dx%d" % s for s in STEM_SHAPES])
@pytest.mark.parametrize("affine", ["engine", "wild"])
def test_stem_input_forms(shape, affine):
    """mnas_stem_fwd / mnas_stem_wgrad with in_u8 and in_affine on the band shapes.  uint8 + affine must equal, bit for bit, the
    plain launch on the float image t that holds the 768-entry table's values (out, the whole stats table, the whole partial
    table); t's results against fp64; float image + affine against fp64 of the fp32-fma staged image; uint8 without an affine
    (the ABI takes it: the conv reads the byte values) bit-identical to the float image of the same integers."""
    lib = L.load()
    N, H, W = shape
    Co = 32
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    wg_band = Wo % 8 == 0
    assert lib.mnas_stem_parts(0, N, H, W, Co) > 0 and (lib.mnas_stem_parts(1, N, H, W, Co) > 0) == wg_band
    gen = torch.Generator(device="cuda").manual_seed(43)
    u8 = torch.randint(0, 256, (N, 3, H, W), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
    u8[0, :, 0, :4] = torch.tensor([0, 255, 1, 254], dtype=torch.uint8, device="cuda")
    w = bf16r(_rand(gen, Co, 3, 3, 3) * (1.0 / 27) ** 0.5)
    wp = pack(w.view(Co, 27, 1, 1), L.PACK_FWD)
    bias = 0.1 * _rand(gen, Co)
    b = _bn(gen, Co)
    g = bf16r(_rand(gen, N, Ho, Wo, Co)).to(torch.bfloat16)
    y = bf16r(_rand(gen, N, Ho, Wo, Co)).to(torch.bfloat16)
    dy64 = bf16r(ref_dy(g, y, b, device="cuda").float()).double()
    aff_h = _engine_affine(True) if affine == "engine" else WILD_AFFINE
    aff = aff_h.cuda().contiguous()
    tab = _staged_table(aff_h).cuda()
    t = torch.stack([tab[c][u8[:, c].long()] for c in range(3)], 1).contiguous()          # (N,3,H,W) fp32 holding bf16 values
    for nparts in (9, lib.mnas_stem_parts(0, N, H, W, Co)):
        oa, sa = _stem_fwd(u8, N, H, W, Co, wp, bias, nparts, aff, 1)
        ot, stt = _stem_fwd(t, N, H, W, Co, wp, bias, nparts)
        bits_equal(oa, ot, "stem_fwd u8+affine vs the staged float image: out (nparts %d)" % nparts)
        bits_equal(sa, stt, "stem_fwd u8+affine vs the staged float image: stats (nparts %d)" % nparts)
        pt = None
        if wg_band:
            np_w = 9 if nparts == 9 else lib.mnas_stem_parts(1, N, H, W, Co)
            pa = _stem_wgrad(u8, N, H, W, Co, grad_in(g, y, b), np_w, aff, 1)
            pt = _stem_wgrad(t, N, H, W, Co, grad_in(g, y, b), np_w)
            bits_equal(pa, pt, "stem_wgrad u8+affine vs the staged float image: partial (nparts %d)" % np_w)
        ref = _stem_check_fp64(t, w, bias, dy64, ot, stt, pt, "stem %s %s nparts %d" % (shape, affine, nparts))
    if not wg_band:            # the fused pipeline exists in the band kernels only: the im2col weight gradient refuses it
        _stem_wgrad(u8, N, H, W, Co, grad_in(g, y, b), 9, aff, 1, expect=L.EINVAL)
    # "pad, then transform" would put `shift` into the padding: with the wild affine that reference must be far outside the tolerance
    # on every border pixel, i.e. the border comparison above can fail
    if affine == "wild":
        tp = torch.zeros((N, 3, H + 2, W + 2), device="cuda") + bf16r(aff[1]).view(1, 3, 1, 1)
        tp[:, :, 1:-1, 1:-1] = t
        wrong = ref_dense_fwd(tp.permute(0, 2, 3, 1), w, bias, stride=2, pad=0, device="cuda")
        assert wrong.shape == ref.shape
        d = ((wrong - ref).abs() / ref.abs().max()).amax(-1)          # per pixel: the worst channel
        assert float(d[:, 0].min()) > 2 * TOL_BF16 and float(d[:, :, 0].min()) > 2 * TOL_BF16, "the padding check cannot fail"
        if H & 1:
            assert float(d[:, -1].min()) > 2 * TOL_BF16
        assert float(d[:, 1:Ho - 1, 1:Wo - 1].max()) < 1e-12
    # float image + affine: staged = bf16(fp32(x*scale + shift)) with ONE rounding to fp32 (fma); no bit claim
    af_h = _engine_affine(False) if affine == "engine" else WILD_AFFINE
    af = af_h.cuda().contiguous()
    xf = torch.rand((N, 3, H, W), generator=gen, device="cuda") * (1.0 if affine == "engine" else 255.0)
    tf = bf16r((xf.double() * af[0].double().view(1, 3, 1, 1) + af[1].double().view(1, 3, 1, 1)).to(torch.float32))
    of, sf = _stem_fwd(xf, N, H, W, Co, wp, bias, 9, af, 0)
    pf = _stem_wgrad(xf, N, H, W, Co, grad_in(g, y, b), 9, af, 0) if wg_band else None
    _stem_check_fp64(tf, w, bias, dy64, of, sf, pf, "stem %s float image + %s affine" % (shape, affine))
    # uint8 without an affine: the conv reads the byte values 0..255 (exact in bf16)
    ou, su = _stem_fwd(u8, N, H, W, Co, wp, bias, 9, None, 1)
    ox, sx = _stem_fwd(u8.float(), N, H, W, Co, wp, bias, 9)
    bits_equal(ou, ox, "stem_fwd u8 without affine vs float bytes: out")
    bits_equal(su, sx, "stem_fwd u8 without affine vs float bytes: stats")
    if wg_band:
        bits_equal(_stem_wgrad(u8, N, H, W, Co, grad_in(g, y, b), 9, None, 1), _stem_wgrad(u8.float(), N, H, W, Co, grad_in(g, y, b), 9),
                   "stem_wgrad u8 without affine vs float bytes: partial")


@pytest.mark.parametrize("shape", [(3, 33, 21, 32), (2, 24, 24, 16), (2, 12, 14, 32)], ids=["W21", "Co16", "W14"])
def test_stem_input_forms_rejected_off_the_band_shapes(shape):
    """W % 4 != 0 or Co != 32: the im2col staging has no fused input pipeline -- MNAS_EINVAL, nothing written"""
    N, H, W, Co = shape
    assert L.load().mnas_stem_parts(0, N, H, W, Co) == -1
    gen = torch.Generator(device="cuda").manual_seed(47)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    u8 = torch.randint(0, 256, (N, 3, H, W), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
    xf = u8.float()
    wp = pack(bf16r(_rand(gen, Co, 27, 1, 1)), L.PACK_FWD)
    aff = _engine_affine(True).cuda()
    g = bf16r(_rand(gen, N, Ho, Wo, Co)).to(torch.bfloat16)
    b = _bn(gen, Co)
    for x, a, flag in ((xf, aff, 0), (u8, aff, 1), (u8, None, 1)):
        _stem_fwd(x, N, H, W, Co, wp, None, 9, a, flag, expect=L.EINVAL)
        _stem_wgrad(x, N, H, W, Co, grad_in(g, g, b), 9, a, flag, expect=L.EINVAL)
    out, _ = _stem_fwd(xf, N, H, W, Co, wp, None, 9)          # the plain float image runs
    assert out is not None


# =====================================================================================================================================
# 1.3  mnas_dw_fwd with a plain input
# =====================================================================================================================================
def _dw_fwd(x, N, H, W, C_, k, stride, wp, bias, nparts, sc=None, sh=None):
    lib = L.load()
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    rows = lib.mnas_dw_rows(N, H, W, C_, k, nparts, 0 if stride == 1 else 4)
    assert 1 <= rows <= nparts, (rows, nparts)
    out, ochk = guarded((N, Ho, Wo, C_), torch.bfloat16)
    st, schk = guarded((2, C_, rows), torch.float32)
    f = L.MnasDwFwd()
    f.N, f.H, f.W, f.C, f.k, f.nparts, f.stride = N, H, W, C_, k, nparts, stride
    f.in_ = act_in(x, sc, sh)
    f.w, f.bias, f.out, f.stats = L.ptr(wp), L.ptr(bias), L.ptr(out), L.ptr(st)
    what = "dw_fwd %s k%d s%d nparts %d (%d rows)%s" % ((N, H, W, C_), k, stride, nparts, rows, " virt" if sc is not None else " plain")
    L.check(lib.mnas_dw_fwd(C.byref(f), L.cur_stream()), what)
    ochk(what + " out")
    schk(what + " stats")
    return out, st, what


def _dw_check(out, st, a, w, bias, k, stride, what, plain, act=None):
    """a: the activated input (N,H,W,C) fp32 (bf16 values when plain); w (C,k,k).  plain (bf16-rounded weights, products exact):
    check_gemm_bound.  Otherwise (fp32 weights as given): check_dw_bound over act_interval of act = (x, scale, shift), or over a
    itself when the input is not virtual, and check_sum_bound on the statistics (the sweep sums its fp32 accumulator)."""
    N = a.shape[0]
    s1 = torch.zeros(a.shape[-1], dtype=torch.float64, device="cuda")
    s2 = torch.zeros_like(s1)
    err, scale = 0.0, 0.0
    sterms = None
    for n0, n1 in _img_chunks(N, a[0].numel()):
        if plain:
            ref = ref_dw_fwd(a[n0:n1], w, bias, stride, device="cuda")
            S = ref_dw_fwd(a[n0:n1].abs(), w.abs(), bias.abs(), stride, device="cuda")
            check_gemm_bound(out[n0:n1], ref, S, k * k, "%s images %d..%d" % (what, n0, n1))
        else:
            iv = act_interval(act[0][n0:n1], act[1], act[2], False, "cuda") if act is not None else Interval.exact(a[n0:n1], "cuda")
            ref, S = dw_fwd_terms(iv, w, bias, stride, "cuda")
            del iv
            check_dw_bound(out[n0:n1], ref, S, k, "%s images %d..%d" % (what, n0, n1), "depthwise forward")
            t = stats_bound_terms(ref, dw_elem_err(S, k))
            sterms = t if sterms is None else tuple(a_ + b_ for a_, b_ in zip(sterms, t))
        del S
        err = max(err, float((out[n0:n1].double() - ref).abs().max()))
        scale = max(scale, float(ref.abs().max()))
        s1 += ref.sum((0, 1, 2))
        s2 += (ref * ref).sum((0, 1, 2))
    assert err / scale < TOL_BF16, (what, err / scale)
    p = st.double().sum(-1)
    assert relerr(p[0], s1) < TOL_F32 and relerr(p[1], s2) < TOL_F32, (what, relerr(p[0], s1), relerr(p[1], s2))
    if sterms is not None:
        Mo, P = out.shape[0] * out.shape[1] * out.shape[2], st.shape[-1]
        check_sum_bound(p[0], sterms[0], sterms[1], Mo, P, 1, what + " stats sum", sterms[2], "depthwise statistics")
        check_sum_bound(p[1], sterms[3], sterms[4], Mo, P, 2, what + " stats sum of squares", sterms[5], "depthwise statistics")


DW_PLAIN = DW + [(2, 12, 12, 48, 5), (2, 13, 14, 72, 3)]


@pytest.mark.parametrize("shape", DW_PLAIN, ids=["%dx%dx%dx%d_k%d" % s for s in DW_PLAIN])
@pytest.mark.parametrize("stride", [1, 2])
def test_dw_fwd_plain_input(shape, stride):
    """scale = shift = NULL: the instance without act-on-load (no ReLU: the inputs are of both signs, so an applied ReLU fails
    the per-element bound); bf16-rounded weights make every product exact in fp32, K = k*k accumulations"""
    N, H, W, C_, k = shape
    gen = torch.Generator(device="cuda").manual_seed(53)
    x = bf16r(_rand(gen, N, H, W, C_))
    w = bf16r(_rand(gen, C_, k, k) * (1.0 / k))
    bias = 0.1 * _rand(gen, C_)
    wp = pack(w.view(C_, 1, k, k), L.PACK_DW)
    xb = x.to(torch.bfloat16)
    outs = []
    for nparts in (40, 173):
        out, st, what = _dw_fwd(xb, N, H, W, C_, k, stride, wp, bias, nparts)
        _dw_check(out, st, x, w, bias, k, stride, what, plain=True)
        outs.append(out)
    bits_equal(outs[1], outs[0], "dw_fwd plain k%d s%d: out across two nparts" % (k, stride))
    assert bool((x < 0).any()) and float(outs[0].min()) < 0


# =====================================================================================================================================
# 1.5  M = 2^24: the pixel decode by exact division
# =====================================================================================================================================
def test_igemm_16m_pixels_split_vs_whole():
    """BASELINE config 5 at batch 256: the SepConv 32 -> 16 project conv over 256 x 256 x 256 = 2^24 pixels runs on k_igemm with
    rcp_hw = 0 (exact integer division in the decode).  Convolution is separable over images and forward output bits do not depend
    on the grid, so the same tensors as two launches of 128 images (2^23 pixels, reciprocal decode) give the reference for every
    element, bit for bit, without fp64 memory; fp64 on 66 images; statistics over all images in chunks.  Then the backward the
    engine launches at that size, mnas_pw_bwd (32 -> 16 is a supported pair, M >= pw_fused_min_pixels): input gradient split versus
    whole, weight gradient against fp64.  Peak: x 1 GB + out 0.5 GB, backward x, gin 1 GB each + g, y 0.5 GB each, fp64 chunks of
    <= 8 images (8 x 2^16 x 32 x 8 B = 134 MB each, a handful alive) and the generator's fp32 temporaries (2 GB): below 8 GB."""
    lib = L.load()
    N, HW, Ci, Co = 256, 256, 32, 16
    M = N * HW * HW
    assert M == 1 << 24
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    gen = torch.Generator(device="cuda").manual_seed(59)
    r = route_of(0, N, HW, HW, Ci, HW, HW, Co, 1, 1, 0, virt=True)
    assert r == ("k_igemm", (1, 2, 32, 0)), r
    x = torch.empty((N, HW, HW, Ci), dtype=torch.bfloat16, device="cuda")
    for n0 in range(0, N, 32):
        x[n0:n0 + 32] = _rand(gen, 32, HW, HW, Ci).to(torch.bfloat16)
    sc, sh = 1 + 0.3 * _rand(gen, Ci), 0.2 * _rand(gen, Ci)
    w = bf16r(_rand(gen, Co, Ci, 1, 1) * (3.0 / Ci) ** 0.5)
    bias = 0.1 * _rand(gen, Co)
    wp = pack(w, L.PACK_FWD)
    nparts = max(1, min(2048, _cdiv(M, 128)))
    whole, st = conv_gemm(0, N, HW, HW, Ci, HW, HW, Co, 1, 1, 0, wp, bias, act=act_in(x, sc, sh), nparts=nparts, stats=True, guard=True)
    for h in (0, 1):
        xs = x[h * 128:(h + 1) * 128]
        assert route_of(0, 128, HW, HW, Ci, HW, HW, Co, 1, 1, 0, virt=True)[0] == "k_igemm"
        half, _ = conv_gemm(0, 128, HW, HW, Ci, HW, HW, Co, 1, 1, 0, wp, bias, act=act_in(xs, sc, sh), nparts=nparts // 2 + 3, stats=True,
                            guard=True)
        bits_equal(whole[h * 128:(h + 1) * 128], half, "2^24-pixel launch vs 2^23-pixel launch, images %d.." % (h * 128))
        del half
    s1 = torch.zeros(Co, dtype=torch.float64, device="cuda")
    s2 = torch.zeros_like(s1)
    picked = {0, N - 1} | {int(round(j * (N - 1) / 63.0)) for j in range(64)}
    for n0 in range(0, N, 8):
        a = bf16r(torch.relu(sc * x[n0:n0 + 8].float() + sh))
        ref = ref_dense_fwd(a, w, bias, 1, 0, device="cuda")
        s1 += ref.sum((0, 1, 2))
        s2 += (ref * ref).sum((0, 1, 2))
        for n in range(n0, n0 + 8):
            if n in picked:
                e = relerr(whole[n].double(), ref[n - n0])
                assert e < TOL_BF16, ("2^24 pixels: image %d" % n, e)
        del a, ref
    p = st.double().sum(-1)
    assert relerr(p[0], s1) < TOL_F32 and relerr(p[1], s2) < TOL_F32, (relerr(p[0], s1), relerr(p[1], s2))
    del whole, st
    torch.cuda.empty_cache()
    # ---- backward as Program._conv_bwd launches it: the fused 1x1 backward
    assert lib.mnas_pw_bwd_supported(Ci, Co) == 1
    bx = _bn(gen, Ci)
    bx[0], bx[1] = sc, sh
    b = _bn(gen, Co)
    g = torch.empty((M, Co), dtype=torch.bfloat16, device="cuda")
    y = torch.empty((M, Co), dtype=torch.bfloat16, device="cuda")
    for m0 in range(0, M, M // 8):
        g[m0:m0 + M // 8] = _rand(gen, M // 8, Co).to(torch.bfloat16)
        y[m0:m0 + M // 8] = _rand(gen, M // 8, Co).to(torch.bfloat16)
    wd = pack(w, L.PACK_DGRAD)
    xm = x.view(M, Ci)

    def pw_bwd(m0, m1, nparts):
        gin, gchk = guarded((m1 - m0, Ci), torch.bfloat16)
        wpart, wchk = guarded((nparts, Co, Ci), torch.float32)
        c = L.MnasPwBwd()
        c.M, c.Ci, c.Co, c.nparts = m1 - m0, Ci, Co, nparts
        c.x, c.dy = act_in(xm[m0:m1], bx[0], bx[1]), grad_in(g[m0:m1], y[m0:m1], b)
        c.w, c.gin, c.wpartial = L.ptr(wd), L.ptr(gin), L.ptr(wpart)
        L.check(lib.mnas_pw_bwd(C.byref(c), L.cur_stream()), "pw_bwd M=%d" % (m1 - m0))
        gchk("pw_bwd M=%d gin" % (m1 - m0))
        wchk("pw_bwd M=%d wpartial" % (m1 - m0))
        return gin, wpart
    npb = max(1, min(1024, _cdiv(M, 128)))
    gin, wpart = pw_bwd(0, M, npb)
    for h in (0, 1):
        gh, _ = pw_bwd(h * (M // 2), (h + 1) * (M // 2), npb // 2 + 3)
        bits_equal(gin[h * (M // 2):(h + 1) * (M // 2)], gh, "pw_bwd 2^24 vs 2^23 pixels: gin, half %d" % h)
        del gh
    grad, chk = guarded((Co, Ci), torch.float32)
    L.check(lib.mnas_wgrad_finalize(L.ptr(wpart), npb, Co, Ci, 1, L.ptr(grad), 0, L.cur_stream()))
    chk("pw_bwd 2^24 dW")
    ref_dw = torch.zeros((Co, Ci), dtype=torch.float64, device="cuda")
    step = 8 * HW * HW
    for m0 in range(0, M, step):
        dy = bf16r(ref_dy(g[m0:m0 + step], y[m0:m0 + step], b, device="cuda").float()).double()
        a = bf16r(torch.relu(sc * xm[m0:m0 + step].float() + sh)).double()
        ref_dw += dy.t() @ a
        if m0 in (0, M - step, M // 2):
            e = relerr(gin[m0:m0 + step].double(), dy @ w.view(Co, Ci).double())
            assert e < TOL_BF16, ("pw_bwd 2^24 gin at pixel %d" % m0, e)
        del dy, a
    assert relerr(grad.double(), ref_dw) < TOL_F32, relerr(grad.double(), ref_dw)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print("\nM = 2^24: forward nparts %d, pw_bwd nparts %d, peak %.1f GB" % (nparts, npb, peak))
    assert peak < 8


# =====================================================================================================================================
# 2.  the forward, weight-gradient, stem and glue launches of the bench configuration's training step, replayed standalone
# =====================================================================================================================================
_CENSUS = {L.OP_CONV_GEMM: "conv_gemm", L.OP_CONV_WGRAD: "conv_wgrad", L.OP_DW_FWD: "dw_fwd", L.OP_STEM_FWD: "stem_fwd",
           L.OP_STEM_WGRAD: "stem_wgrad", L.OP_BN_BWD_REDUCE: "bn_bwd_reduce", L.OP_ADD_ACT: "add_act", L.OP_POOL_ACT: "pool_act",
           L.OP_POOL_BWD: "pool_bwd"}
_FORM_SLOTS = {   # pointer slots (by their names in _lib.OP_SLOTS) whose presence selects a form
    L.OP_CONV_GEMM: {"virt": "act.scale", "dy.y": "grad.y", "bias": "bias", "resid": "resid", "stats": "stats", "red": "red_y",
                     "gate": "gate"},
    L.OP_CONV_WGRAD: {"virt": "x.scale", "dy.y": "dy.y"}, L.OP_DW_FWD: {"virt": "in_.scale", "bias": "bias", "stats": "stats"},
    L.OP_STEM_FWD: {"bias": "bias", "stats": "stats", "affine": "in_affine"}, L.OP_STEM_WGRAD: {"dy.y": "dy.y", "affine": "in_affine"},
    L.OP_BN_BWD_REDUCE: {}, L.OP_ADD_ACT: {"a.virt": "a.scale", "b": "b.data", "b.virt": "b.scale", "out": "out_bf16", "nchw": "out_nchw"},
    L.OP_POOL_ACT: {"virt": "a.scale"}, L.OP_POOL_BWD: {},
}


def _census(prog, seen, finalize):
    """distinct (opcode, integers, pointer-presence flags) over the forward list and every backward segment; `finalize` collects
    the (nsplit, Co, Ci, taps) of the WGRAD_FINALIZE / BWD_POST slots, which every CONV_WGRAD launch must have a match in"""
    lists = [(prog.fwd_ops, prog.fwd_n)] + [(arr, n) for _, arr, n in prog.bwd_segments]
    for arr, n in lists:
        for j in range(n):
            o = arr[j]
            if o.opcode == L.OP_WGRAD_FINALIZE:
                finalize.add(tuple(int(L.op_field(o, n)) for n in ("nsplit", "Co", "Ci", "taps")))
            if o.opcode == L.OP_BWD_POST:
                for w in ("w1.", "w2."):
                    if L.op_field(o, w + "level") and not L.op_field(o, w + "dw"):
                        finalize.add(tuple(int(L.op_field(o, w + n)) for n in ("nsplit", "Co", "Ci", "taps")))
            if o.opcode not in _CENSUS:
                continue
            ints = L.op_ints(o)
            if o.opcode in (L.OP_BN_BWD_REDUCE, L.OP_ADD_ACT):
                ints = ints + (int(L.op_field(o, "rows")),)
            flags = tuple(sorted((k, bool(L.op_field(o, s))) for k, s in _FORM_SLOTS[o.opcode].items()))
            key = (o.opcode, ints, flags)
            seen[key] = seen.get(key, 0) + 1


def _gemm_from_ints(ints, flags, gen):
    mode, N = ints[0], ints[1]
    k, stride, pad, nparts = ints[8], ints[10], ints[11], ints[12]
    assert ints[8] == ints[9] and pad == k // 2 and not flags["gate"]
    if mode == 0:
        Hi, Wi, Ci, Ho, Wo, Co = ints[2:8]
        cs = _GemmCase(0, N, Hi, Wi, Ci, Co, k, stride, gen, virt=flags["virt"], bias=flags["bias"])
        assert not flags["resid"]
    else:
        Ho, Wo, Co, Hi, Wi, Ci = ints[2:8]
        cs = _GemmCase(1, N, Hi, Wi, Ci, Co, k, stride, gen, coef=flags["dy.y"], resid=flags["resid"], red=flags["red"])
    assert (cs.Ho, cs.Wo) == (Ho, Wo), (ints, cs.Ho, cs.Wo)
    return cs, nparts


def _replay_gemm(ints, flags, gen):
    lib = L.load()
    cs, nparts = _gemm_from_ints(ints, flags, gen)
    r, inst = cs.route()
    # the grid the engine must have asked the library for
    M = cs.N * cs.Ho * cs.Wo if cs.mode == 0 else cs.N * cs.H * cs.W
    K1 = cs.Ci if cs.mode == 0 else cs.Co
    N1 = cs.Co if cs.mode == 0 else cs.Ci
    pref = lib.mnas_conv_gemm_parts(cs.mode, M, K1, N1, cs.k * cs.k)
    if cs.k == 3 and not (cs.mode == 1 and (flags["dy.y"] or flags["resid"])):
        a = (0, cs.N, cs.H, cs.W, cs.Ci, cs.Ho, cs.Wo, cs.Co) if cs.mode == 0 else (1, cs.N, cs.Ho, cs.Wo, cs.Co, cs.H, cs.W, cs.Ci)
        ip = lib.mnas_conv_img_parts(*a, cs.k, cs.stride, cs.pad)
        pref = ip if ip > 0 else pref
    if pref > 0:
        assert nparts == pref, (cs.what(), "nparts", nparts, "library's preferred grid", pref)
    out, st = cs.launch(nparts, stats=flags.get("stats", True))
    rel, worst = cs.check(out, st)
    alt = max(1, nparts // 2 + 3)
    out2, st2 = cs.launch(alt, stats=flags.get("stats", True))
    bits_equal(out2, out, cs.what() + ": out vs nparts %d" % alt)
    if st is not None:        # the statistics / fused-reduce columns depend on the grid, their sums only by rounding
        e = relerr(st2.double().sum(-1), st.double().sum(-1))
        assert e < TOL_F32, (cs.what(), "column sums, nparts %d vs %d" % (alt, nparts), e)
    return r, inst, "nparts %d / %d  err %.1e%s" % (nparts, alt, rel, "  bound x%.2f" % worst if cs.plain else "")


def _replay_wgrad(ints, flags, gen):
    lib = L.load()
    N, Hi, Wi, Ci, Ho, Wo, Co, k, _, stride, pad, nsp = ints
    slabs = lib.mnas_conv_wgrad_slabs(Co, Ci, k * k)
    assert 1 <= nsp and nsp * slabs <= 512 and nsp <= _cdiv(N * Ho * Wo, 256), (ints, slabs)
    assert nsp == max(1, min(512 // slabs, _cdiv(N * Ho * Wo, 256))), (ints, slabs)
    x = bf16r(_rand(gen, N, Hi, Wi, Ci)).to(torch.bfloat16)
    sc, sh = 1 + 0.3 * _rand(gen, Ci), 0.2 * _rand(gen, Ci)
    g = bf16r(_rand(gen, N, Ho, Wo, Co)).to(torch.bfloat16)
    y = bf16r(_rand(gen, N, Ho, Wo, Co)) if flags["dy.y"] else None
    b = _bn(gen, Co) if flags["dy.y"] else None
    if y is not None:
        y = _off_hinge(y, b[0], b[1]).to(torch.bfloat16)             # (dy's mask input: the per-element bound below needs the device's mask bits)
    part, pchk = guarded((nsp, Co, k * k * Ci), torch.float32)
    a = L.MnasConvWgrad()
    a.N, a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.Co = N, Hi, Wi, Ci, Ho, Wo, Co
    a.kh = a.kw = k
    a.stride, a.pad, a.nsplit = stride, pad, nsp
    a.x = act_in(x, sc if flags["virt"] else None, sh if flags["virt"] else None)
    a.dy, a.partial = grad_in(g, y, b), L.ptr(part)
    what = "conv_wgrad %s" % (ints,)
    L.check(lib.mnas_conv_wgrad(C.byref(a), L.cur_stream()), what)
    pchk(what + " partial")
    grad, gchk = guarded((Co, Ci, k, k), torch.float32)
    L.check(lib.mnas_wgrad_finalize(L.ptr(part), nsp, Co, Ci, k * k, L.ptr(grad), 0, L.cur_stream()))
    gchk(what + " dW")
    ref = torch.zeros((Co, Ci, k, k), dtype=torch.float64, device="cuda")
    # check_sum_bound (c = 1) over the operands' bf16 intervals, chunk by chunk: ref over the interval mids, S over the largest
    # magnitudes, slack = S - sum |mid||mid| (bounds_conv.wgrad_terms, accumulated over the image chunks)
    r64, S, Sm = torch.zeros_like(ref), torch.zeros_like(ref), torch.zeros_like(ref)
    for n0, n1 in _img_chunks(N, max(Hi * Wi * Ci, Ho * Wo * Co)):
        xs = x[n0:n1].float()
        act = bf16r(torch.relu(sc * xs + sh)) if flags["virt"] else xs
        dy = bf16r(ref_dy(g[n0:n1], y[n0:n1], b, device="cuda").float()) if flags["dy.y"] else g[n0:n1].float()
        ref += ref_dense_wgrad(act, dy, k, stride, pad, device="cuda")
        aiv = act_interval(xs, sc, sh, True, "cuda") if flags["virt"] else Interval.exact(xs, "cuda")
        div = dy_interval(g[n0:n1].float(), y[n0:n1].float(), b, True, "cuda") if flags["dy.y"] else Interval.exact(g[n0:n1].float(), "cuda")
        r64 += ref_dense_wgrad(aiv.mid, div.mid, k, stride, pad, device="cuda")
        S += ref_dense_wgrad(aiv.amax, div.amax, k, stride, pad, device="cuda")
        Sm += ref_dense_wgrad(aiv.mid.abs(), div.mid.abs(), k, stride, pad, device="cuda")
        del aiv, div
    e = relerr(grad.double(), ref)
    assert e < TOL_F32, (what, "dW", e)
    worst = check_sum_bound(grad, r64, S, N * Ho * Wo, nsp, 1, what + " dW", (S - Sm).clamp_min(0), "weight gradient (replayed)")
    return "nsplit %d x %d slabs  err %.1e  bound x%.3f" % (nsp, slabs, e, worst)


def _replay_dw(ints, flags, gen):
    N, H, W, C_, k, nlaunch, stride = ints
    stride = max(1, stride)
    x = bf16r(_rand(gen, N, H, W, C_))
    sc, sh = 1 + 0.3 * _rand(gen, C_), 0.2 * _rand(gen, C_)
    w = _rand(gen, C_, k, k) * (1.0 / k)
    bias = 0.1 * _rand(gen, C_) if flags["bias"] else None
    wp = pack(w.view(C_, 1, k, k), L.PACK_DW)
    xb = x.to(torch.bfloat16)
    virt = flags["virt"]
    a = torch.relu(sc * x + sh) if virt else x               # act-on-read: fp32, not re-rounded
    out, st, what = _dw_fwd(xb, N, H, W, C_, k, stride, wp, bias, nlaunch, sc if virt else None, sh if virt else None)
    zb = torch.zeros(C_, device="cuda") if bias is None else bias
    _dw_check(out, st, a, w, zb, k, stride, what, plain=False, act=(x, sc, sh) if virt else None)
    alt = nlaunch // 2 + 3
    out2, st2, _ = _dw_fwd(xb, N, H, W, C_, k, stride, wp, bias, alt, sc if virt else None, sh if virt else None)
    bits_equal(out2, out, what + ": out vs nparts %d" % alt)
    return "nlaunch %d (%d rows) / %d (%d rows)" % (nlaunch, st.shape[-1], alt, st2.shape[-1])


def _replay_stem(fwd_ints, wg_ints, flags, gen):
    """both stem launches of one Program on the same image; uint8 + affine: bit-identical to the staged float image"""
    lib = L.load()
    N, H, W, Ho, Wo, Co, nparts, in_u8 = fwd_ints
    assert Co == 32 and nparts == lib.mnas_stem_parts(0, N, H, W, Co) and nparts > 0, "the stem is not on its band kernel / grid"
    assert wg_ints[:6] == fwd_ints[:6] and wg_ints[7] == in_u8 and wg_ints[6] == min(lib.mnas_stem_parts(1, N, H, W, Co), 768)
    assert bool(flags["affine"]) == bool(in_u8), "the bench configuration normalises on the device exactly when it feeds uint8"
    w = bf16r(_rand(gen, Co, 3, 3, 3) * (1.0 / 27) ** 0.5)
    wp = pack(w.view(Co, 27, 1, 1), L.PACK_FWD)
    bias = 0.1 * _rand(gen, Co) if flags["bias"] else None
    b = _bn(gen, Co)
    g = bf16r(_rand(gen, N, Ho, Wo, Co)).to(torch.bfloat16)
    y = bf16r(_rand(gen, N, Ho, Wo, Co)).to(torch.bfloat16)
    dy64 = bf16r(ref_dy(g, y, b, device="cuda").float()).double()
    if in_u8:
        aff_h = _engine_affine(True)
        aff = aff_h.cuda().contiguous()
        u8 = torch.randint(0, 256, (N, 3, H, W), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
        tab = _staged_table(aff_h).cuda()
        t = torch.stack([tab[c][u8[:, c].long()] for c in range(3)], 1).contiguous()
        oa, sa = _stem_fwd(u8, N, H, W, Co, wp, bias, nparts, aff, 1)
        pa = _stem_wgrad(u8, N, H, W, Co, grad_in(g, y, b), wg_ints[6], aff, 1)
    else:
        t = bf16r(_rand(gen, N, 3, H, W))
    ot, stt = _stem_fwd(t, N, H, W, Co, wp, bias, nparts)
    pt = _stem_wgrad(t, N, H, W, Co, grad_in(g, y, b), wg_ints[6])
    if in_u8:
        bits_equal(oa, ot, "stem_fwd u8+affine vs staged float image: out")
        bits_equal(sa, stt, "stem_fwd u8+affine vs staged float image: stats")
        bits_equal(pa, pt, "stem_wgrad u8+affine vs staged float image: partial")
        del oa, sa, pa
    _stem_check_fp64(t, w, bias, dy64, ot, stt, pt, "stem %s" % (fwd_ints,))
    alt = nparts // 2 + 3
    o2, _ = _stem_fwd(t, N, H, W, Co, wp, bias, alt)
    bits_equal(o2, ot, "stem_fwd out vs nparts %d" % alt)
    return "fwd nparts %d / %d, wgrad nparts %d" % (nparts, alt, wg_ints[6])


def _replay_bn_reduce(ints, flags, gen):
    C_, nred, rows = ints
    lib = L.load()
    b = _bn(gen, C_)
    g = bf16r(_rand(gen, rows, C_)).to(torch.bfloat16)
    y = _off_hinge(bf16r(_rand(gen, rows, C_)), b[0], b[1]).to(torch.bfloat16)
    part, chk = guarded((2, C_, nred), torch.float32)
    L.check(lib.mnas_bn_bwd_reduce(L.ptr(g), L.ptr(y), L.ptr(b), rows, C_, nred, L.ptr(part), L.cur_stream()), "bn_bwd_reduce")
    chk("bn_bwd_reduce %s" % (ints,))
    _check_red(part, g.float(), y.float(), b, "bn_bwd_reduce %s" % (ints,))
    return "nred %d" % nred


def _act64(x, sc, sh):
    return torch.relu(sc.double() * x.double() + sh.double()) if sc is not None else x.double()


def _replay_add_act(ints, flags, gen):
    C_, HW, rows = ints
    lib = L.load()
    xa, xb = bf16r(_rand(gen, rows, C_)).to(torch.bfloat16), bf16r(_rand(gen, rows, C_)).to(torch.bfloat16)
    sa, ta, sb, tb = 1 + 0.3 * _rand(gen, C_), 0.2 * _rand(gen, C_), 1 + 0.3 * _rand(gen, C_), 0.2 * _rand(gen, C_)
    A = act_in(xa, sa if flags["a.virt"] else None, ta if flags["a.virt"] else None)
    B = act_in(xb, sb if flags["b.virt"] else None, tb if flags["b.virt"] else None) if flags["b"] else None
    ref = _act64(xa, sa if flags["a.virt"] else None, ta)
    if flags["b"]:
        ref = ref + _act64(xb, sb if flags["b.virt"] else None, tb)
    out, ochk = guarded((rows, C_), torch.bfloat16) if flags["out"] else (None, None)
    Nn = rows // HW
    nchw, nchk = guarded((Nn, C_, HW), torch.float32) if flags["nchw"] else (None, None)
    L.check(lib.mnas_add_act(C.byref(A), C.byref(B) if B is not None else None, rows, C_, L.ptr(out), L.ptr(nchw), HW, L.cur_stream()), "add_act")
    what = "add_act %s" % (ints,)
    if out is not None:
        ochk(what + " out")
        err = (out.double() - ref).abs()
        assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-6).all()), (what, "bf16 out beyond one rounding of the fp64 sum", float(err.max()))
    if nchw is not None:
        nchk(what + " nchw")
        assert relerr(nchw.double(), ref.view(Nn, HW, C_).permute(0, 2, 1)) < 1e-6, what
    return ""


def _replay_pool_act(ints, flags, gen):
    N, HW, C_ = ints
    lib = L.load()
    x = bf16r(_rand(gen, N, HW, C_)).to(torch.bfloat16)
    sc, sh = 1 + 0.3 * _rand(gen, C_), 0.2 * _rand(gen, C_)
    A = act_in(x, sc if flags["virt"] else None, sh if flags["virt"] else None)
    out, chk = guarded((N, C_), torch.float32)
    L.check(lib.mnas_pool_act(C.byref(A), N, HW, C_, L.ptr(out), L.cur_stream()), "pool_act")
    chk("pool_act %s" % (ints,))
    ref = _act64(x, sc if flags["virt"] else None, sh).mean(1)
    assert relerr(out.double(), ref) < 1e-5, ("pool_act", ints, relerr(out.double(), ref))
    return ""


def _replay_pool_bwd(ints, flags, gen):
    N, HW, C_ = ints
    lib = L.load()
    gp = _rand(gen, N, C_)
    g, chk = guarded((N, HW, C_), torch.bfloat16)
    L.check(lib.mnas_pool_bwd(L.ptr(gp), N, HW, C_, L.ptr(g), L.cur_stream()), "pool_bwd")
    chk("pool_bwd %s" % (ints,))
    ref = (gp.double() / HW).view(N, 1, C_).expand(N, HW, C_)
    err = (g.double() - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs()).all()), ("pool_bwd", ints, float(err.max()))
    return ""


def test_bench_config_forward_wgrad_stem_launches():
    """BASELINE configs[1] as bench.py runs it (ccf=False, head '512', bs 256, 224x224, training), once with float images and once
    with uint8 images after normalize_on_device(): every distinct CONV_GEMM (both modes), CONV_WGRAD, DW_FWD, STEM_FWD / STEM_WGRAD,
    BN_BWD_REDUCE, ADD_ACT, POOL_ACT and POOL_BWD launch of the two Programs replayed on its own with the production integers, on
    device-generated operands, against fp64 on the device; outputs bit-identical on a second grid.

    Expected from the engine code (Program._conv_fwd / _conv_bwd and the library's plan functions) and asserted:
      forward 1x1: the expand convs 16->48 at 112^2 and 24->72 at 56^2 on k_pwf (M >= 400 000: its 128-pixel tiles), their plain
      inputs (a residual sum) where the block repeats; the widening convs of the <= 28^2 maps on k_pwx (40->240, 80->480, 96->576);
      the long reductions on k_pws (K >= 192, M <= 250 000); the narrowing convs of the large maps on k_igemm;
      forward 3x3: 16->24 at 112^2 and 24->40 at 56^2 on k_c3x, 40->80 at 28^2 -> 14^2 on k_dimg (stride 2), 80->96 at 14^2 on
      k_dimg, 96->192 and 192->320 on k_c3r, all three whole-image kernels at N = 256;
      forward 1x1 on k_igemm: the narrowing convs of the 112^2 / 56^2 maps (32->16, 48->16, 72->24);
      input gradients through mnas_conv_gemm: a materialised dy for every dense 3x3 that the transposed-conv kernels do not take
      (192<-320 at 7^2 on k_c3r, 80<-96 at 14^2 on k_dimg, the stride-2 40<-80 on k_igemm's parity-class form), dy-on-load with
      K >= 192 on k_pws (with the residual and the fused reduce), 1152<-192 on k_igemm;
      nparts of every launch equal to mnas_conv_gemm_parts / mnas_conv_img_parts where those return > 0; the stem on its band
      kernels with mnas_stem_parts grids, with in_u8 and in_affine set together in the uint8 Program;
      every CONV_WGRAD with nsplit = min(512 // slabs, M / 256) and a WGRAD_FINALIZE or BWD_POST slot of the same (nsplit, Co, Ci, taps)."""
    import contextlib
    import io
    from mnasnet_pytorch_amd import FineTuneModelPool, load_model
    from mnasnet_pytorch_amd.train_step import Trainer
    N, HW = 256, 224
    seen, finalize, stem = {}, set(), {}
    for u8 in (False, True):
        with contextlib.redirect_stdout(io.StringIO()):
            base = load_model("mnasnet")
        m = FineTuneModelPool(base, "mnasnet", 1000, "512").cuda().train()
        if u8:
            m.normalize_on_device()
        tr = Trainer(m, lr=1e-3)
        eng = tr.engine
        eng.ensure_setup(torch.device("cuda"))
        eng._check_modes()
        prog = eng.program(N, HW, HW, True, False, True, u8)
        one = {}
        _census(prog, one, finalize)
        if u8:
            aff = eng.input_affine(True)
            assert aff is not None and torch.equal(aff.cpu(), _engine_affine(True)), "Engine.input_affine(uint8) is not 1/(255 std), -mean/std"
        for k, v in one.items():
            seen[k] = seen.get(k, 0) + v
        stem[u8] = ([k for k in one if k[0] == L.OP_STEM_FWD], [k for k in one if k[0] == L.OP_STEM_WGRAD])
        del prog
        eng.reset_programs()
        del tr, eng, m, base
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    lib = L.load()
    keys = sorted(seen, key=lambda k: (k[0], k[1], k[2]))
    gen = torch.Generator(device="cuda").manual_seed(2027)
    lines, routes = [], {}
    for u8 in (False, True):
        assert len(stem[u8][0]) == 1 and len(stem[u8][1]) == 1, stem[u8]
        f, wg = stem[u8]
        fl = dict(f[0][2])
        fl["dy.y"] = dict(wg[0][2])["dy.y"]
        assert dict(wg[0][2])["affine"] == fl["affine"]
        torch.cuda.synchronize()
        info = _replay_stem(f[0][1], wg[0][1], fl, gen)
        torch.cuda.empty_cache()
        lines.append("%-44s ints %-52s %s" % ("stem fwd+wgrad%s" % (" u8 affine" if u8 else " float"), f[0][1], info))
    for k in keys:
        opc, ints, flags = k[0], k[1], dict(k[2])
        if opc in (L.OP_STEM_FWD, L.OP_STEM_WGRAD):
            continue
        form = _CENSUS[opc] + "".join(" " + n for n, v in sorted(flags.items()) if v)
        torch.cuda.synchronize()
        if opc == L.OP_CONV_GEMM:
            r, inst, info = _replay_gemm(ints, flags, gen)
            routes.setdefault((ints[0], r), []).append((ints, flags, inst))
            form = "conv_gemm mode %d %s%s%s" % (ints[0], r, " %s" % (inst,) if r == "k_igemm" else "", form[len("conv_gemm"):])
        elif opc == L.OP_CONV_WGRAD:
            assert (ints[11], ints[6], ints[3], ints[7] * ints[8]) in finalize, ("CONV_WGRAD without its finalize slot", ints)
            info = _replay_wgrad(ints, flags, gen)
        elif opc == L.OP_DW_FWD:
            info = _replay_dw(ints, flags, gen)
        elif opc == L.OP_BN_BWD_REDUCE:
            info = _replay_bn_reduce(ints, flags, gen)
        elif opc == L.OP_ADD_ACT:
            info = _replay_add_act(ints, flags, gen)
        elif opc == L.OP_POOL_ACT:
            info = _replay_pool_act(ints, flags, gen)
        else:
            info = _replay_pool_bwd(ints, flags, gen)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        lines.append("%-44s ints %-52s x%d  %s" % (form[:44], ints, seen[k], info))
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print("\nbench-config forward / weight-gradient / stem census (%d distinct launches over the float and the uint8 Program; replay "
          "peak %.1f GB):\n  %s" % (len(lines), peak, "\n  ".join(lines)))
    # ---- what the engine code says this configuration launches
    def chans(mode, route):
        return {(i[4], i[7]) for i, _, _ in routes.get((mode, route), [])}
    assert chans(0, "k_pwf") >= {(16, 48), (24, 72)}, chans(0, "k_pwf")
    assert all(i[1] * i[5] * i[6] >= 400000 for i, _, _ in routes[(0, "k_pwf")] if (i[4], i[7]) in ((16, 48), (24, 72))), "k_pwf 128-pixel tiles"
    assert any(not f["virt"] for _, f, _ in routes[(0, "k_pwf")]), "no expand conv reading a plain residual sum"
    assert chans(0, "k_pwx") >= {(40, 240), (80, 480), (96, 576)}, chans(0, "k_pwx")
    assert chans(0, "k_pws") and all(c[0] >= 192 for c in chans(0, "k_pws")), chans(0, "k_pws")
    assert chans(0, "k_c3x") >= {(16, 24), (24, 40)}, chans(0, "k_c3x")
    assert (40, 80) in chans(0, "k_dimg") and any(i[10] == 2 for i, _, _ in routes[(0, "k_dimg")]), chans(0, "k_dimg")
    assert chans(0, "k_c3r") >= {(192, 320)}, chans(0, "k_c3r")
    assert all(i[1] == N for r in ("k_dimg", "k_c3r") for i, _, _ in routes[(0, r)])
    assert chans(0, "k_igemm") >= {(32, 16), (48, 16), (72, 24)}, chans(0, "k_igemm")          # the narrowing convs of the 112^2 / 56^2 maps
    # input gradients (channels: dy, result): the 7x7 / 14x14 dense convs on the whole-image kernels over a materialised dy, the
    # stride-2 40 -> 80 conv (which no transposed-conv kernel takes: 4*Co > 256) on k_igemm's parity-class form
    assert chans(1, "k_c3r") >= {(320, 192)} and chans(1, "k_dimg") >= {(96, 80)}, (chans(1, "k_c3r"), chans(1, "k_dimg"))
    assert any(inst[3] == 1 and (i[4], i[7]) == (80, 40) for i, _, inst in routes[(1, "k_igemm")]), routes[(1, "k_igemm")]
    assert chans(1, "k_pws") and all(c[0] >= 192 for c in chans(1, "k_pws")), chans(1, "k_pws")
    assert all(not f["dy.y"] for r in ("k_c3r", "k_dimg") for _, f, _ in routes[(1, r)])
    assert peak < 20


def test_c3x_16m_pixels_split_vs_whole():
    """k_c3x carries the same decode switch: 16 -> 24, stride 2, 256 images of 512 x 512 -> 256 x 256 = 2^24 output pixels in one
    launch against the same tensors as two launches of 128 images (2^23 pixels, reciprocal decode), bit for bit; fp64 on three
    images; statistics sums of the whole against the halves.  x 2 GB + out 0.75 GB + a half's out: peak below 8 GB."""
    N, H, Ci, Co = 256, 512, 16, 24
    Ho = H // 2
    assert N * Ho * Ho == 1 << 24
    assert route_of(0, N, H, H, Ci, Ho, Ho, Co, 3, 2, 1, virt=True)[0] == "k_c3x"
    assert route_of(0, N // 2, H, H, Ci, Ho, Ho, Co, 3, 2, 1, virt=True)[0] == "k_c3x"
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    gen = torch.Generator(device="cuda").manual_seed(61)
    x = torch.empty((N, H, H, Ci), dtype=torch.bfloat16, device="cuda")
    for n0 in range(0, N, 16):
        x[n0:n0 + 16] = _rand(gen, 16, H, H, Ci).to(torch.bfloat16)
    sc, sh = 1 + 0.3 * _rand(gen, Ci), 0.2 * _rand(gen, Ci)
    w = bf16r(_rand(gen, Co, Ci, 3, 3) * (3.0 / (9 * Ci)) ** 0.5)
    bias = 0.1 * _rand(gen, Co)
    wp = pack(w, L.PACK_FWD)
    whole, st = conv_gemm(0, N, H, H, Ci, Ho, Ho, Co, 3, 2, 1, wp, bias, act=act_in(x, sc, sh), nparts=1024, stats=True, guard=True)
    sums = torch.zeros((2, Co), dtype=torch.float64, device="cuda")
    for h in (0, 1):
        half, sth = conv_gemm(0, N // 2, H, H, Ci, Ho, Ho, Co, 3, 2, 1, wp, bias, act=act_in(x[h * 128:(h + 1) * 128], sc, sh), nparts=515,
                              stats=True, guard=True)
        bits_equal(whole[h * 128:(h + 1) * 128], half, "k_c3x 2^24-pixel launch vs 2^23-pixel launch, images %d.." % (h * 128))
        sums += sth.double().sum(-1)
        del half
    assert relerr(st.double().sum(-1), sums) < TOL_F32, relerr(st.double().sum(-1), sums)
    for n in (0, 127, N - 1):
        a = bf16r(torch.relu(sc * x[n:n + 1].float() + sh))
        ref = ref_dense_fwd(a, w, bias, 2, 1, device="cuda")
        e = relerr(whole[n:n + 1].double(), ref)
        assert e < TOL_BF16, ("k_c3x 2^24 pixels: image %d" % n, e)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print("\nk_c3x M = 2^24: peak %.1f GB" % peak)
    assert peak < 8
