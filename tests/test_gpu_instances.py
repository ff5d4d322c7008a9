"""-m gpu: one launch per reachable template instantiation of the conv kernel families (tests/instance_cases.py), each under the
per-element bounds of tests/bounds_conv.py and the machinery of the existing kernel tests -- nothing is re-derived here:

  conv_gemm families   test_gpu_fwd_forms._GemmCase: check_gemm_bound / check_onload_bound, forward statistics and fused-reduce
                       bounds, guarded buffers, bit identity of the output on a second grid
  gated k_pws          as test_gpu_se.test_gated_project_forward: bit identity with the launch on the materialised product of
                       mnas_se_scale, check_onload_bound over gated_act_interval, check_stats_bound
  k_wgrad_t            test_gpu_fwd_forms._replay_wgrad: mnas_conv_wgrad + finalize, check_sum_bound with c = 1
  k_tcx/k_tcr/k_tconv  test_gpu_bwd_forms.test_tconv_dgrad, plain and with the fused reduce
  k_pw_bwd             test_gpu_bwd_forms._PwCase (the bounds of test_pw_bwd_fused)
  depthwise sweeps     test_gpu_fwd_forms._replay_dw (forward), test_gpu_bwd_forms._DwCase (backward, every phase)

Every launch is preceded by the library's own instance query on the very struct that is launched (the entry points are wrapped for
the duration of a case), and the case asserts that the instance it names ran.  Each case prints `family instance error / bound`:
the largest measured error over its bound among all the per-element and per-sum checks of the case."""
import ctypes as C
from contextlib import contextmanager

import pytest
import torch

import instance_cases as IC
import intervals
from bounds_conv import check_onload_bound, check_stats_bound, onload_elem_err, onload_fwd_terms
from bounds_se import gate_nhwc, gated_act_interval, sigmoid_interval
from gpu_util import L, act_in, bits_equal, conv_gemm, pack
from test_gpu_bwd_forms import _DwCase, _PwCase, _cdiv
from test_gpu_bwd_forms import test_tconv_dgrad as _tconv_dgrad_body
from test_gpu_bwd_forms import _replay_dw as _replay_dw_bwd
from test_gpu_fwd_forms import _GemmCase, _replay_dw as _replay_dw_fwd, _replay_wgrad

pytestmark = pytest.mark.gpu
WORST = {}          # family -> (largest error / bound, the case's id)


# ---- the instance of every launch, asked on the struct that is launched -------------------------------------------------------------
def _gemm_inst(a):
    r = IC.gemm_instance_of(a)
    return None if r is None else r[:2]


def _tconv_inst(a):
    out = (C.c_int * 8)()
    r = L.load().mnas_tconv_dgrad_instance(C.byref(a), out)
    if r < 0:
        return None
    fam = IC.TCONV_KERNELS[r]
    return fam, tuple(out[:3] if fam == "k_tcr" else out[:2])


def _wgrad_inst(a):
    out = (C.c_int * 2)()
    return ("k_wgrad_t", tuple(out)) if L.load().mnas_conv_wgrad_instance(C.byref(a), out) == 0 else None


def _pw_bwd_inst(a):
    out = (C.c_int * 8)()
    return ("k_pw_bwd", (out[0], out[1], out[2], out[4], out[5])) if L.load().mnas_pw_bwd_instance(C.byref(a), out) == 0 else None


def _dw_fwd_inst(a):
    r = IC.dw_instance_of(a.N, a.H, a.W, a.C, a.k, 0) if a.stride in (0, 1) else None
    return None if r is None else r[:2]


def _dw_bwd_inst(a):
    r = IC.dw_instance_of(a.N, a.H, a.W, a.C, a.k, a.phase + 1) if a.stride in (0, 1) else None
    return None if r is None else r[:2]


_ENTRY = {"mnas_conv_gemm": _gemm_inst, "mnas_tconv_dgrad": _tconv_inst, "mnas_conv_wgrad": _wgrad_inst, "mnas_pw_bwd": _pw_bwd_inst,
          "mnas_dw_fwd": _dw_fwd_inst, "mnas_dw_bwd": _dw_bwd_inst}


@contextmanager
def _launched():
    """wraps the launch entry points of the loaded library: yields the list of (family, instance) of every launch made inside"""
    lib = L.load()
    seen = []
    real = {name: getattr(lib, name) for name in _ENTRY}

    def wrap(name):
        def call(ref, stream):
            seen.append(_ENTRY[name](ref._obj))
            return real[name](ref, stream)
        return call
    try:
        for name in _ENTRY:
            setattr(lib, name, wrap(name))
        yield seen
    finally:
        for name, fn in real.items():
            setattr(lib, name, fn)


# ---- conv_gemm families ---------------------------------------------------------------------------------------------------------------
class _Case(_GemmCase):
    """_GemmCase over the operands instance_cases.gemm_operands built on the CPU (the tensors the CPU test has checked)"""
    def __init__(self, spec):
        mode, N, H, W, Ci, Co, k, stride, form = spec
        o = {n: (None if t is None else t.cuda()) for n, t in IC.gemm_operands(spec).items()}
        self.mode, self.N, self.H, self.W, self.Ci, self.Co, self.k, self.stride = mode, N, H, W, Ci, Co, k, stride
        self.pad = k // 2
        self.Ho, self.Wo = (H + 2 * self.pad - k) // stride + 1, (W + 2 * self.pad - k) // stride + 1
        self.virt, self.coef = form.get("virt", True), form.get("coef", True)
        self.w = o["w"]
        self.wp = pack(self.w, L.PACK_FWD if mode == 0 else L.PACK_DGRAD)
        self.bias = self.resid = self.y_in = self.b_in = None
        if mode == 0:
            self.x, self.sc, self.sh, self.bias = o["x"].to(torch.bfloat16), o["sc"], o["sh"], o["bias"]
            self.u = o.get("u")
        else:
            self.g = o["g"].to(torch.bfloat16)
            self.b = o.get("b")
            self.y = o["y"].to(torch.bfloat16) if self.coef else None
            if "resid" in o:
                self.resid = o["resid"].to(torch.bfloat16)
            if "y_in" in o:
                self.b_in, self.y_in = o["b_in"], o["y_in"].to(torch.bfloat16)


def _grids(M):
    return (13, 38) if M < 100000 else (96, 331)


def _run_gemm(case):
    family, inst, spec = case
    cs = _Case(spec)
    assert cs.route()[0] == family
    M = cs.N * cs.Ho * cs.Wo if cs.mode == 0 else cs.N * cs.H * cs.W
    worst, outs = 0.0, []
    for p in ((5, 17) if cs.k == 3 and family != "k_c3x" else _grids(M)):
        out, st = cs.launch(p)
        worst = max(worst, cs.check(out, st)[1])
        outs.append(out)
    bits_equal(outs[1], outs[0], cs.what() + ": out vs another grid")
    return worst


def _run_gated(case):
    """the squeeze-excite gate on load: bit-identical to the launch on the product mnas_se_scale materialises; per-element and
    statistics bounds over the gated operand's interval"""
    family, inst, spec = case
    lib = L.load()
    cs = _Case(spec)
    N, H, W, Ci, Co = cs.N, cs.H, cs.W, cs.Ci, cs.Co
    M = N * H * W
    assert lib.mnas_conv_gemm_gate_ok(N, H * W, Ci, Co) == 1
    gate = torch.full((N, Ci), float("nan"), device="cuda")
    L.check(lib.mnas_se_gate(cs.u.data_ptr(), N, Ci, gate.data_ptr(), L.cur_stream()), "se_gate")
    a2s = torch.empty((N, H, W, Ci), dtype=torch.bfloat16, device="cuda")
    ai = act_in(cs.x, cs.sc, cs.sh)
    L.check(lib.mnas_se_scale(C.byref(ai), cs.u.data_ptr(), N, H * W, Ci, a2s.data_ptr(), L.cur_stream()), "se_scale")
    iv = gated_act_interval(cs.x.float(), cs.sc, cs.sh, gate_nhwc(sigmoid_interval(cs.u, "cuda"), cs.x.shape), True, "cuda")
    r64, slack, S = onload_fwd_terms(iv, cs.w, cs.bias, device="cuda")
    what = "gated 1x1 forward %s" % (spec[:8],)
    worst, outs = 0.0, []
    for nparts in _grids(M):
        out_g, st_g = conv_gemm(0, N, H, W, Ci, H, W, Co, 1, 1, 0, cs.wp, bias=cs.bias, act=ai, nparts=nparts, stats=True, gate=gate, guard=True)
        with _launched() as plain:
            out_m, st_m = conv_gemm(0, N, H, W, Ci, H, W, Co, 1, 1, 0, cs.wp, bias=cs.bias, act=act_in(a2s), nparts=nparts, stats=True, guard=True)
        assert plain == [(family, inst[:4] + (0,))], ("the materialised twin runs the same instance without the gate", plain)
        bits_equal(out_g, out_m, what + ": out, gate on load vs materialised")
        bits_equal(st_g, st_m, what + ": statistics, gate on load vs materialised")
        worst = max(worst, check_onload_bound(out_g, r64, slack, S, Ci, what, "gated 1x1 forward"))
        worst = max(worst, check_stats_bound(st_g, r64, onload_elem_err(slack, S, Ci), M, what, "forward statistics (gated)"))
        outs.append(out_g)
    bits_equal(outs[1], outs[0], what + ": out vs another grid")
    return worst


# ---- the other entry points ---------------------------------------------------------------------------------------------------------
def _run_wgrad(case):
    N, H, W, Ci, Co, k = case[2]
    slabs = L.load().mnas_conv_wgrad_slabs(Co, Ci, k * k)
    nsp = max(1, min(512 // slabs, _cdiv(N * H * W, 256)))
    assert nsp > 1 and (N * H * W) % nsp != 0          # several pixel splits, the last one ragged
    gen = torch.Generator(device="cuda").manual_seed(67)
    _replay_wgrad((N, H, W, Ci, H, W, Co, k, k, 1, k // 2, nsp), {"virt": True, "dy.y": True}, gen)
    return 0.0


def _run_tconv(case):
    family, inst, (N, Ho, Wo, Co, Ci) = case
    kernel = {("k_tcx", (1, 3)): "tcx13", ("k_tcx", (2, 5)): "tcx25", ("k_tcr", (2, 3, 6)): "tcr", ("k_tconv", (2, 1)): "tconv"}[(family, inst)]
    for fused_red in (False, True):
        _tconv_dgrad_body((kernel, N, Ho, Wo, Co, Ci), fused_red)
    return 0.0


def _run_pw_bwd(case):
    N, H, W, Ci, Co, form = case[2]
    M = N * H * W
    gen = torch.Generator(device="cuda").manual_seed(71)
    cs = _PwCase(M, Ci, Co, gen, virt=True, bias=(form == "recomp"))
    kw = {"red": dict(red=True), "recomp": dict(red=True),
          "red_other": dict(red=True, red_y=cs.x.clone())}[form]      # (a copy of x: the same reduce, but not the out-stage form's operand)
    if form == "recomp":
        wf = pack(cs.w.view(Co, Ci, 1, 1), L.PACK_FWD)
        nfp = L.load().mnas_conv_gemm_parts(0, M, Ci, Co, 1)
        y, _ = conv_gemm(0, N, H, W, Ci, H, W, Co, 1, 1, 0, wf, cs.bias, act=act_in(cs.x, cs.bx[0], cs.bx[1]), nparts=max(1, nfp))
        cs.set_y(y.view(M, Co))
        kw["recomp"] = (wf, cs.bias)
    outs = []
    for nparts in (3, 7):
        r = cs.launch(nparts, **kw)
        cs.check_ref(*r)
        outs.append(r)
    bits_equal(outs[1][0], outs[0][0], outs[0][3] + ": gin vs another grid")
    if form == "recomp":
        s = cs.launch(3, red=True)
        bits_equal(outs[0][0], s[0], outs[0][3] + ": gin RECOMP vs stored y")
        bits_equal(outs[0][1], s[1], outs[0][3] + ": wpartial RECOMP vs stored y")
    return 0.0


def _dw_phase(cs, nparts, phase):
    """one launch of phase 1 (input gradient + reduce) or 2 (weight gradient) in guarded buffers"""
    from gpu_util import grad_in, guarded
    lib = L.load()
    d = L.MnasDwBwd()
    d.N, d.H, d.W, d.C, d.k, d.nparts, d.phase = cs.N, cs.H, cs.W, cs.C, cs.k, nparts, phase
    d.x, d.dy, d.w = act_in(cs.x, cs.bx[0], cs.bx[1]), grad_in(cs.g, cs.y, cs.b), L.ptr(cs.wp)
    rows = lib.mnas_dw_rows(cs.N, cs.H, cs.W, cs.C, cs.k, nparts, phase + 1)
    assert rows >= 1
    what = "dw_bwd %s k%d nparts %d phase %d" % ((cs.N, cs.H, cs.W, cs.C), cs.k, nparts, phase)
    if phase == 1:
        gin, gchk = guarded((cs.N, cs.H, cs.W, cs.C), torch.bfloat16)
        redp, rchk = guarded((2, cs.C, rows), torch.float32)
        d.gin, d.red_bn, d.red_partial = L.ptr(gin), L.ptr(cs.bx), L.ptr(redp)
        L.check(lib.mnas_dw_bwd(C.byref(d), L.cur_stream()), what)
        gchk(what + " gin")
        rchk(what + " red_partial")
        return gin, redp, rows, what
    wpart, wchk = guarded((rows, cs.k * cs.k, cs.C), torch.float32)
    d.wpartial = L.ptr(wpart)
    L.check(lib.mnas_dw_bwd(C.byref(d), L.cur_stream()), what)
    wchk(what + " wpartial")
    return wpart, rows, what


def _run_dw(case):
    family, inst, (N, H, W, C_) = case
    ks = inst[0]
    gen = torch.Generator(device="cuda").manual_seed(73)
    if family == "k_dw_fwd":
        _replay_dw_fwd((N, H, W, C_, ks, 40, 1), {"bias": True, "virt": True}, gen)
    elif inst[1] == 0:
        _replay_dw_bwd((N, H, W, C_, ks, 37, 0, 1, 0), {"red": True}, gen, N)
    else:       # the two-launch form: phase 1 and phase 2 together give what _DwCase.check_ref checks
        cs = _DwCase(N, H, W, C_, ks, gen)
        gins = []
        for nparts in (37, 11):
            gin, redp, _, what = _dw_phase(cs, nparts, 1)
            wpart, rows, _ = _dw_phase(cs, nparts, 2)
            cs.check_ref((gin, wpart, redp, rows, what + "+2"))
            gins.append(gin)
        bits_equal(gins[1], gins[0], what + ": gin vs another grid")
    return 0.0


RUN = {"k_wgrad_t": _run_wgrad, "k_tcx": _run_tconv, "k_tcr": _run_tconv, "k_tconv": _run_tconv, "k_pw_bwd": _run_pw_bwd,
       "k_dw_fwd": _run_dw, "k_dw_bwd": _run_dw}


def _check_case(case):
    family, inst, spec = case
    assert IC.instance_of(*case)[:2] == (family, inst)
    saved = dict(intervals.WORST)
    intervals.WORST.clear()
    try:
        with _launched() as seen:
            if family in IC.ROUTES:
                worst = _run_gated(case) if spec[8].get("gate") else _run_gemm(case)
            else:
                worst = RUN[family](case)
        assert None not in seen, "a launch the instance query refuses went through"
        assert (family, inst) in seen, ("the named instance never ran", sorted(set(seen)))
        if family in IC.ROUTES:         # (a gated case also launches its twin on the materialised product)
            allowed = {(family, inst), (family, inst[:4] + (0,))} if spec[8].get("gate") else {(family, inst)}
            assert set(seen) <= allowed, ("a launch of the case ran another instance", sorted(set(seen)))
        worst = max([worst] + list(intervals.WORST.values()))
    finally:
        for f, v in saved.items():
            intervals.WORST[f] = max(intervals.WORST.get(f, 0.0), v)
    assert 0.0 < worst <= 1.0
    print("%s %s error / bound %.3f" % (family, inst, worst))
    if worst > WORST.get(family, (0.0, ""))[0]:
        WORST[family] = (worst, IC.case_id(case))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", IC.CASES, ids=[IC.case_id(c) for c in IC.CASES])
def test_instance(case):
    _check_case(case)


@pytest.mark.parametrize("case", IC.FINDINGS, ids=["%dx%dx%dx%d_%d_m%d" % (c[2][1:6] + (c[2][0],)) for c in IC.FINDINGS])
def test_finding(case):
    """shapes that ran on an instance too small for them (k_c3r with more than 24 k-steps per wave), where they run now"""
    _check_case(case)


def test_worst_error_over_bound_per_family():
    """the summary DESIGN.md section 6 records (a measurement, not a target: every bound was asserted case by case)"""
    for family in sorted(WORST):
        print("%-10s worst error / bound %.3f (%s)" % (family, WORST[family][0], WORST[family][1]))
