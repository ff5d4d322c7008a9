"""One launch per reachable template instantiation of every conv kernel family that picks its instance on the host.

CASES holds (family, instance, spec): the smallest shape found by the sweep of tests/test_instances_cpu.py that reaches the
instance, with a pixel count that is no multiple of the instance's pixel tile and -- where the plan admits one -- a channel count
that leaves the last cout tile ragged.  UNREACHABLE holds the instantiations that no argument reaches, each with its arithmetic.
PLAN_UNREACHABLE names plan values that would pick another code path inside an instance but that the default build never produces.
No GPU at import: the host-side queries of include/mnas.h (mnas_*_instance, mnas_dw_geometry) resolve a spec to its instance.

Instance tuples per family (the template arguments the host picks):
  k_pws (MODE, NT, KSW, NW, GATE)   k_pwf (NT, PT, WRES)   k_pwd (NT, PT)   k_pwx (TPW, KS, NW)   k_dimg (MODE, PXW, CG)
  k_c3r (MODE, NT, KSW, PTW, KQ)    k_c3x (TPW, KS)        k_igemm (MODE, NT, PT)
  k_tcx (TPW, KSM)   k_tcr (KQ0, KQ1, KQ3)   k_tconv (NT, PT)   k_wgrad_t (CT, KT)   k_pw_bwd (NTO, NTI, PT, OS, FORM)
  k_dw_fwd (KS, G)   k_dw_bwd (KS, phase, G)

Specs:
  conv_gemm families  (mode, N, H, W, Ci, Co, k, stride, form): the conv (N,H,W,Ci) -> Co, mode 1 = its input gradient (form: the
                      keyword arguments of test_gpu_fwd_forms._GemmCase; "gate": the squeeze-excite gate on load)
  k_tcx/k_tcr/k_tconv (N, Ho, Wo, Co, Ci) as test_gpu_bwd_forms.TCONV
  k_wgrad_t           (N, H, W, Ci, Co, k)
  k_pw_bwd            (N, H, W, Ci, Co, form) with form in "red" (fused reduce against x itself), "red_other" (against a copy of x:
                      the plain epilogue), "recomp"
  k_dw_fwd, k_dw_bwd  (N, H, W, C)"""
import ctypes as C

import torch

from mnasnet_pytorch_amd import _lib as L

V, P = dict(virt=True), dict(virt=False)
DC, DM = dict(coef=True, red=True), dict(coef=False, red=True)
DR = dict(coef=True, resid=True, red=True)
G = dict(virt=True, gate=True)

PX = (3, 11, 13)            # 429 pixels: 26 16-pixel groups + 13, 6 64-pixel tiles + 45, 3 128-pixel tiles + 45
PX2 = (25, 127, 127)        # 403 225 pixels (k_pwf / k_pwd / k_tconv take 128-pixel tiles from 400 000): 3150 tiles + 25
PXI = (33, 63, 65)          # 135 135 pixels (k_igemm takes 128-pixel tiles from 131 072 x cout blocks): 1055 tiles + 95

CASES = []


def _add(family, inst, spec):
    CASES.append((family, tuple(inst), spec))


# ---- k_pws: K = reduction length >= 192; NT = 3 up to 3 cout tiles, else 6; 8 waves from 21 k-steps (mode 1: from 12)
for nt, n in ((3, 8), (6, 56)):          # 8 of 48 / 56 of 96 outputs: the last tile ragged
    for ksw, nw, K in ((2, 4, 200), (3, 4, 264), (5, 4, 392), (3, 8, 648), (5, 8, 776)):
        _add("k_pws", (0, nt, ksw, nw, 0), (0,) + PX + (K, n, 1, 1, V))
        if ksw <= 3:
            _add("k_pws", (0, nt, ksw, nw, 1), (0,) + PX + (K, n, 1, 1, G))
    for ksw, nw, K in ((2, 4, 200), (3, 4, 264), (2, 8, 392), (3, 8, 520)):
        _add("k_pws", (1, nt, ksw, nw, 0), (1,) + PX + (n, K, 1, 1, DR if nt == 3 else DC))
# ---- k_pwf (widening, Ci <= 128) / k_pwd: NT = cout tiles up to 6
for nt in range(1, 7):
    co = 16 if nt == 1 else 16 * nt - 8                  # (Co > Ci = 8 leaves no ragged tile for NT = 1)
    _add("k_pwf", (nt, 1, 1), (0,) + PX + (8, co, 1, 1, V))
    _add("k_pwf", (nt, 2, 1), (0,) + PX2 + (8, co, 1, 1, V))
    _add("k_pwd", (nt, 1), (1,) + PX + (co, 8, 1, 1, dict(coef=True, red=True)))
    if nt <= 4:
        _add("k_pwd", (nt, 2), (1,) + PX2 + (co, 8, 1, 1, dict(coef=True, red=True)))
# weights not resident: only where the 128-pixel form with resident weights exceeds 96 KB of LDS, and the plan then falls back to
# 64-pixel tiles -- M >= 400 000 and Kpad >= 96 (NT 4, 5) or 64 (NT 6)
_add("k_pwf", (4, 1, 0), (0,) + PX2 + (72, 104, 1, 1, V))          # (7 cout tiles: two blocks of 4)
_add("k_pwf", (5, 1, 0), (0,) + PX2 + (72, 136, 1, 1, V))          # (9 cout tiles: two blocks of 5)
_add("k_pwf", (6, 1, 0), (0,) + PX2 + (40, 88, 1, 1, V))
# ---- k_pwx: 40 -> 240, 80 -> 480, 96 -> 576 and their neighbours
_add("k_pwx", (4, 2, 4), (0,) + PX + (40, 200, 1, 1, V))
_add("k_pwx", (5, 3, 6), (0,) + PX + (72, 392, 1, 1, V))
_add("k_pwx", (6, 3, 6), (0,) + PX + (72, 520, 1, 1, V))
# ---- k_dimg: PXW by the pixels of a pass (<= 64, <= 128, <= 256), CG = cout tiles per group (bound 3 / 6 with PXW 4, else 12)
for mode, form in ((0, V), (1, DM)):
    io = (lambda ci, co: (ci, co)) if mode == 0 else (lambda ci, co: (co, ci))
    _add("k_dimg", (mode, 1, 12), (mode, 33, 3, 3) + io(16, 8) + (3, 1, form))            # two images per pass (ni = 2), odd N
    _add("k_dimg", (mode, 2, 12), (mode, 32, 9, 9) + io(40, 8) + (3, 1, form))            # two K chunks (nkc = 2)
    _add("k_dimg", (mode, 4, 3), (mode, 33, 12, 11) + io(16, 8) + (3, 1, form))
    _add("k_dimg", (mode, 4, 6), (mode, 33, 12, 11) + io(16, 824) + (3, 1, form))
_add("k_dimg", (0, 2, 12), (0, 33, 6, 7, 32, 8, 3, 1, V))                                 # ni = 2 and nkc = 2 together
# ---- k_c3r: planes <= 64 pixels, 9*Ci*Co >= 128 K; every plan has more than one cout slice
_add("k_c3r", (0, 2, 14, 2, 4), (0, 33, 5, 5, 152, 104, 3, 2, V))                         # stride 2 only (see UNREACHABLE)
_add("k_c3r", (0, 3, 7, 4, 8), (0, 33, 3, 4, 152, 104, 3, 1, V))
_add("k_c3r", (0, 2, 12, 4, 8), (0, 33, 3, 4, 200, 88, 3, 1, V))
_add("k_c3r", (1, 3, 7, 4, 8), (1, 33, 3, 4, 104, 152, 3, 1, DM))
_add("k_c3r", (1, 2, 12, 4, 8), (1, 33, 3, 4, 72, 208, 3, 1, DM))
# ---- k_c3x: stride 2, at least 100 000 output pixels
_add("k_c3x", (2, 5), (0, 9, 221, 213, 8, 24, 3, 2, V))
_add("k_c3x", (3, 7), (0, 9, 221, 213, 24, 40, 3, 2, V))
# ---- k_igemm (MODE, NT, PT): what no other family takes
for nt, c in ((1, 8), (2, 24), (3, 40), (4, 56), (6, 72), (8, 104)):
    _add("k_igemm", (0, nt, 1), (0,) + PX + (c, c, 1, 1, V))
    _add("k_igemm", (0, nt, 2), (0,) + PXI + (c, c, 1, 1, V))
    _add("k_igemm", (1, nt, 1), (1,) + PX + (c, 8, 1, 1, DR))
    _add("k_igemm", (1, nt, 2), (1,) + PXI + (c, 8, 1, 1, DR))
# ---- transposed convs
_add("k_tcx", (1, 3), (3, 13, 9, 24, 16))
_add("k_tcx", (2, 5), (3, 13, 9, 40, 24))
_add("k_tcr", (2, 3, 6), (33, 6, 7, 192, 112))
_add("k_tconv", (2, 1), (2, 9, 11, 48, 8))
# ---- k_wgrad_t: CT x 32 couts by KT x 32 k per slab
for ct in range(1, 6):
    for kt in range(1, 5):
        if (ct, kt) != (5, 4):
            _add("k_wgrad_t", (ct, kt), PX + (32 * kt - 24, 32 * ct - 24, 1))
_add("k_wgrad_t", (1, 4), PX + (24, 8, 3))                 # the same slab shapes through the 3x3 gather
_add("k_wgrad_t", (2, 3), PX + (8, 40, 3))
# ---- k_pw_bwd: the supported channel pairs; OS = out-stage form (fused reduce against x itself, no residual), FORM 2 = RECOMP
for (nto, nti, pt), (ci, co) in (((1, 2, 2), (32, 16)), ((1, 3, 2), (48, 16)), ((3, 1, 2), (16, 48)), ((5, 2, 1), (24, 72)),
                                  ((2, 5, 2), (72, 24)), ((15, 3, 1), (40, 240)), ((3, 5, 1), (240, 40)), ((5, 5, 1), (480, 80)),
                                  ((6, 6, 1), (576, 96)), ((8, 3, 1), (40, 120)), ((3, 4, 1), (120, 40))):
    os_form = (nti > nto and nti >= 3) or (nti == nto and nti >= 5)
    _add("k_pw_bwd", (nto, nti, pt, 0, 0), PX + (ci, co, "red_other" if os_form else "red"))
    if os_form:
        _add("k_pw_bwd", (nto, nti, pt, 1, 0), PX + (ci, co, "red"))
    if nto > nti and nti <= 2:
        _add("k_pw_bwd", (nto, nti, pt, 0, 2), PX + (ci, co, "recomp"))
# ---- depthwise sweeps: G = rows per DMA group; 7 rows (no multiple of either G), 5 columns (one ragged 4-column strip pair)
for ks, c4, c2 in ((3, 40, {0: 168, 1: 256, 2: 168}), (5, 40, {0: 112, 1: 216, 2: 112})):
    _add("k_dw_fwd", (ks, 4), (2, 7, 5, c4))
    for phase in (0, 1, 2):
        _add("k_dw_bwd", (ks, phase, 4), (2, 7, 5, c4))
        _add("k_dw_bwd", (ks, phase, 2), (2, 7, 5, c2[phase]))

# shapes an earlier planner sent to an instance that cannot hold them (see UNREACHABLE, k_c3r): where they run now, same bounds
FINDINGS = [
    ("k_dimg", (0, 1, 12), (0, 33, 3, 4, 344, 56, 3, 1, V)),
    ("k_dimg", (1, 1, 12), (1, 33, 3, 4, 56, 344, 3, 1, DM)),
    ("k_dimg", (0, 2, 12), (0, 33, 7, 7, 392, 56, 3, 1, V)),
]

UNREACHABLE = [
    # k_pws: pws_plan takes 8 waves from 21 k-steps (mode 1: from 12), so a wave's slice is ceil(21 / 8) = 3 steps (mode 1:
    # ceil(12 / 8) = 2 is possible) -- KSW = 2 with NW = 8 never forward, gated or not
    ("k_pws", (0, 3, 2, 8, 0), "NW = 8 needs more than 20 k-steps, i.e. at least ceil(21/8) = 3 per wave"),
    ("k_pws", (0, 6, 2, 8, 0), "NW = 8 needs more than 20 k-steps, i.e. at least ceil(21/8) = 3 per wave"),
    ("k_pws", (0, 3, 2, 8, 1), "as the plain twin"), ("k_pws", (0, 6, 2, 8, 1), "as the plain twin"),
    ("k_pws", (1, 3, 5, 4, 0), "pws_plan refuses mode 1 with more than 3 k-steps per wave"),
    ("k_pws", (1, 6, 5, 4, 0), "pws_plan refuses mode 1 with more than 3 k-steps per wave"),
    ("k_pws", (1, 3, 5, 8, 0), "pws_plan refuses mode 1 with more than 3 k-steps per wave"),
    ("k_pws", (1, 6, 5, 8, 0), "pws_plan refuses mode 1 with more than 3 k-steps per wave"),
    # k_pwf: the default build takes Ci <= 128 only, one K chunk; non-resident weights (two chunk buffers) then need MORE LDS
    # than resident ones (one), so WRES = 0 is only ever chosen on the way from PT = 2 down to PT = 1, and only where
    # pwf_lds_bytes(0, NT, 2, Kpad <= 128, ...) exceeds 96 KB: NT >= 4
    ("k_pwf", (1, 1, 0), "LDS of the resident 128-pixel form <= 96 KB for NT <= 3 at Kpad <= 128"),
    ("k_pwf", (2, 1, 0), "LDS of the resident 128-pixel form <= 96 KB for NT <= 3 at Kpad <= 128"),
    ("k_pwf", (3, 1, 0), "LDS of the resident 128-pixel form <= 96 KB for NT <= 3 at Kpad <= 128"),
    ("k_pwf", (1, 2, 0), "with one K chunk WRES = 0 only grows the LDS: the plan goes on to PT = 1"),
    ("k_pwf", (2, 2, 0), "with one K chunk WRES = 0 only grows the LDS: the plan goes on to PT = 1"),
    ("k_pwf", (3, 2, 0), "with one K chunk WRES = 0 only grows the LDS: the plan goes on to PT = 1"),
    ("k_pwf", (4, 2, 0), "with one K chunk WRES = 0 only grows the LDS: the plan goes on to PT = 1"),
    ("k_pwf", (5, 2, 0), "with one K chunk WRES = 0 only grows the LDS: the plan goes on to PT = 1"),
    ("k_pwf", (6, 2, 0), "with one K chunk WRES = 0 only grows the LDS: the plan goes on to PT = 1"),
    # k_pwd: pwf_lds_bytes(1, 5, 2, 32, 32, 1, 1) = 84 096 > 80 KB already at the shortest K
    ("k_pwd", (5, 2), "128-pixel tiles with 5 cout tiles need 84 096 B of LDS at Kpad = 32, the budget is 80 KB"),
    ("k_pwd", (6, 2), "128-pixel tiles with 6 cout tiles need more LDS than with 5"),
    # k_c3r: NT = 2 with KSW = 14 means <= 56 k-steps (Ci <= 192) and not the three-tile form, i.e. ceil(Co/48) == ceil(Co/32):
    # Co <= 32 or 49..64, where 9*Ci*Co <= 9*192*64 = 110 592 < 128 K.  Mode 0 reaches it at stride 2 (no three-tile form there).
    ("k_c3r", (1, 2, 14, 2, 4), "stride 1 sends every weight-heavy shape with <= 56 k-steps to the three-tile form"),
    # NT = 1 means more than 14 k-steps per wave of the 4-way split, i.e. at least 57 k-steps; up to 96 k-steps the 8-way split with
    # two cout tiles (KQ = 8, KSW = 12) takes the shape, and 97 k-steps are ceil(97/4) = 25 per wave: more than the 24 fragments.
    # (c3r_plan accepted 25..28 per wave before: a (0, 1, 24, 2, 4) case with Ci = 344 missed its bound 28-fold; see FINDINGS.)
    ("k_c3r", (0, 1, 24, 2, 4), "57..96 k-steps go to the 8-way split, 97 and more exceed 24 per wave"),
    ("k_c3r", (1, 1, 24, 2, 4), "57..96 k-steps go to the 8-way split, 97 and more exceed 24 per wave"),
    # k_tconv: NT = ceil(4*Ci/16) with Ci a multiple of 8 is even; k_tcx takes every Co <= 40 with Ci <= 32, and from Co = 48 the
    # staged tiles (2*64 + NT*16 rows of Kpad/8 + 1 = 25 chunks) fit the 80 KB budget for NT = 2 and Co = 48 alone
    ("k_tconv", (3, 1), "NT is even"), ("k_tconv", (3, 2), "NT is even"), ("k_tconv", (5, 1), "NT is even"), ("k_tconv", (5, 2), "NT is even"),
    ("k_tconv", (4, 1), "Co >= 48 (below: k_tcx): (128 + 64) * 25 * 16 + 16 384 B > 80 KB"),
    ("k_tconv", (6, 1), "Co >= 48 (below: k_tcx): more LDS than NT = 4"),
    ("k_tconv", (2, 2), "Co >= 48: (256 + 32) * 25 * 16 B = 115 200 > 80 KB"),
    ("k_tconv", (4, 2), "more LDS than (2, 2)"), ("k_tconv", (6, 2), "more LDS than (2, 2)"),
    # depthwise forward: one ring; with 8-row rings 32 * iw * cpw <= 32 * (4 * 256 + 4 * 128) B = 48 KB is under the 78 KB cap for
    # every candidate, so the 4-row search finds the same best geometry with the same score and 0.93 * score never wins
    ("k_dw_fwd", (3, 2), "the LDS cap never binds with one ring: G = 2 scores the same and loses the 0.93 tie-break"),
    ("k_dw_fwd", (5, 2), "the LDS cap never binds with one ring: G = 2 scores the same and loses the 0.93 tie-break"),
]

PLAN_UNREACHABLE = [
    ("k_pwf", "nkc > 1", "the default build routes Ci <= 128 here (pwf_plan), i.e. Kpad <= 128 = one chunk"),
    ("k_tcx", "nblocks > 1", "the channel block is min(16 * TPW, Ci) and the plan takes Ci <= 16 * TPW"),
    ("k_c3r", "slices == 1", "one slice needs Co <= 48, then 9*Ci*Co >= 128 K needs Ci >= 304, where no slab shape fits"),
]

ROUTES = ["k_pwx", "k_pws", "k_pwf", "k_pwd", "k_c3r", "k_dimg", "k_c3x", "k_igemm"]          # MNAS_ROUTE_*
TCONV_KERNELS = ["k_tcx", "k_tcr", "k_tconv"]                                                    # MNAS_TCONV_*


# ---- host-side queries --------------------------------------------------------------------------------------------------------------
def gemm_instance_of(a):
    """(family, instance tuple, raw int[8]) of a filled MnasConvGemm, or None where the launch refuses it"""
    out = (C.c_int * 8)()
    r = L.load().mnas_conv_gemm_instance(C.byref(a), out)
    if r < 0:
        return None
    fam, o = ROUTES[r], tuple(out)
    inst = {"k_pws": (a.mode,) + o[:4], "k_pwf": o[:3], "k_pwd": o[:2], "k_pwx": o[:3], "k_dimg": (a.mode,) + o[:2],
            "k_c3r": (a.mode,) + o[:4], "k_c3x": o[:2], "k_igemm": (a.mode,) + o[:2]}[fam]
    return fam, inst, o


def gemm_struct(mode, N, H, W, Ci, Co, k, stride, virt=True, coef=True, resid=False, red=False, bias=True, gate=False, one=64):
    """MnasConvGemm of the spec's conv with `one` standing for every pointer the form sets (nothing is dereferenced by a query)"""
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    a = L.MnasConvGemm()
    a.mode, a.N = mode, N
    if mode == 0:
        a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.Co = H, W, Ci, Ho, Wo, Co
        a.act = L.MnasActIn(one, one if virt else 0, one if virt else 0)
        a.bias = one if bias else 0
        a.stats = one
    else:
        a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.Co = Ho, Wo, Co, H, W, Ci
        a.grad = L.MnasGradIn(one, one if coef else 0, one if coef else 0)
        if red:
            a.red_y = a.red_bn = a.stats = one
    a.kh = a.kw = k
    a.stride, a.pad, a.nparts = stride, pad, 64
    a.resid = one if resid else 0
    a.gate = one if gate else 0
    a.w = a.out = one
    return a


def tconv_instance_of(N, Ho, Wo, Co, Ci):
    t = L.MnasTconvDgrad()
    t.N, t.Ho, t.Wo, t.Co, t.Ci, t.nparts = N, Ho, Wo, Co, Ci, 8
    t.dy = t.w = t.out = 64
    out = (C.c_int * 8)()
    r = L.load().mnas_tconv_dgrad_instance(C.byref(t), out)
    if r < 0:
        return None
    fam = TCONV_KERNELS[r]
    return fam, tuple(out[:3] if fam == "k_tcr" else out[:2]), tuple(out)


def wgrad_instance_of(N, H, W, Ci, Co, k):
    w = L.MnasConvWgrad()
    w.N, w.Hi, w.Wi, w.Ci, w.Ho, w.Wo, w.Co = N, H, W, Ci, H, W, Co
    w.kh = w.kw = k
    w.stride, w.pad, w.nsplit = 1, k // 2, 1
    out = (C.c_int * 2)()
    r = L.load().mnas_conv_wgrad_instance(C.byref(w), out)
    return None if r < 0 else ("k_wgrad_t", tuple(out), tuple(out))


PW_BWD_FORMS = {"red": dict(red=1), "red_other": dict(red=2), "recomp": dict(red=1, recomp=1)}


def pw_bwd_instance_of(M, Ci, Co, red=0, resid=0, recomp=0, masked=0):
    """red: 1 = fused reduce against x itself, 2 = against another tensor"""
    p = L.MnasPwBwd()
    p.M, p.Ci, p.Co, p.nparts = M, Ci, Co, 8
    p.x = L.MnasActIn(64, 64, 64)
    p.dy = L.MnasGradIn(64, 0 if recomp else 64, 64)
    p.w = p.gin = p.wpartial = 64
    p.resid = 64 if resid else 0
    if red:
        p.red_partial = p.red_bn = 64
        p.red_y = 64 if red == 1 else 128
    p.w_fwd = 64 if recomp else 0
    p.gin_masked = masked
    out = (C.c_int * 8)()
    r = L.load().mnas_pw_bwd_instance(C.byref(p), out)
    return None if r < 0 else ("k_pw_bwd", (out[0], out[1], out[2], out[4], out[5]), tuple(out))


def dw_instance_of(N, H, W, C_, ks, which):
    """which as in mnas_dw_geometry: 0 forward, 1 / 2 / 3 = backward phase 0 / 1 / 2"""
    g = (C.c_int * 7)()
    if L.load().mnas_dw_geometry(N, H, W, C_, ks, which, g) != 0:
        return None
    return ("k_dw_fwd", (ks, g[6]), tuple(g)) if which == 0 else ("k_dw_bwd", (ks, which - 1, g[6]), tuple(g))


def instance_of(family, inst, spec):
    """the (family, instance, raw plan values) the library picks for a case's launch"""
    if family in ROUTES:
        mode, N, H, W, Ci, Co, k, s, form = spec
        return gemm_instance_of(gemm_struct(mode, N, H, W, Ci, Co, k, s, **form))
    if family in TCONV_KERNELS:
        return tconv_instance_of(*spec)
    if family == "k_wgrad_t":
        return wgrad_instance_of(*spec)
    if family == "k_pw_bwd":
        N, H, W, Ci, Co, form = spec
        return pw_bwd_instance_of(N * H * W, Ci, Co, **PW_BWD_FORMS[form])
    if family == "k_dw_fwd":
        return dw_instance_of(*spec, inst[0], 0)
    if family == "k_dw_bwd":
        return dw_instance_of(*spec, inst[0], inst[1] + 1)
    raise KeyError(family)


def case_id(case):
    family, inst, _ = case
    return "%s_%s" % (family, "_".join(str(v) for v in inst))


def case_elements(case):
    """elements of the case's largest tensor pair (operand + result)"""
    family, _, spec = case
    if family in ROUTES:
        mode, N, H, W, Ci, Co, k, s, _ = spec
        p = k // 2
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        return N * H * W * Ci + N * Ho * Wo * Co
    if family in TCONV_KERNELS:
        N, Ho, Wo, Co, Ci = spec
        return N * Ho * Wo * (Co + 4 * Ci)
    if family in ("k_wgrad_t", "k_pw_bwd"):
        return spec[0] * spec[1] * spec[2] * (spec[3] + spec[4])
    return 3 * spec[0] * spec[1] * spec[2] * spec[3]


# ---- operands of the conv_gemm cases: built on the CPU from the case's own seed, so that the CPU test sees the very tensors the
# GPU test launches with (tests/test_gpu_instances.py moves them to the device)
def _u(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def _bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _bn(gen, C_):
    b = torch.zeros(8, C_)
    b[0], b[1] = 1 + 0.3 * _u(gen, C_), 0.2 * _u(gen, C_)
    b[2], b[3], b[4] = b[0], 0.05 * _u(gen, C_), 0.02 * _u(gen, C_)
    b[5], b[6] = 0.1 * _u(gen, C_), 1 + 0.2 * _u(gen, C_).abs()
    return b


def gemm_operands(spec, seed=61):
    """fp32 CPU tensors holding bf16 values, distributed as test_gpu_fwd_forms._GemmCase draws them; y and y_in are moved off the
    ReLU hinge (bounds_conv.off_hinge asserts its share limit)"""
    from bounds_conv import off_hinge
    mode, N, H, W, Ci, Co, k, s, form = spec
    gen = torch.Generator().manual_seed(seed)
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    o = dict(w=_bf16r(_u(gen, Co, Ci, k, k) * (3.0 / (k * k * (Ci if mode == 0 else Co))) ** 0.5))
    if mode == 0:
        o["x"] = _bf16r(_u(gen, N, H, W, Ci))
        o["sc"], o["sh"] = 1 + 0.3 * _u(gen, Ci), 0.2 * _u(gen, Ci)
        o["bias"] = 0.1 * _u(gen, Co) if form.get("bias", True) else None
        if form.get("gate"):
            o["u"] = 2.0 * _u(gen, N, Ci)                       # the gate's pre-activation (mnas_se_gate takes its sigmoid)
    else:
        o["g"] = _bf16r(_u(gen, N, Ho, Wo, Co))
        if form.get("coef", True):
            o["b"] = _bn(gen, Co)
            o["y"] = off_hinge(_bf16r(_u(gen, N, Ho, Wo, Co)), o["b"][0], o["b"][1])
        if form.get("resid"):
            o["resid"] = _bf16r(_u(gen, N, H, W, Ci))
        if form.get("red"):
            o["b_in"] = _bn(gen, Ci)
            o["y_in"] = off_hinge(_bf16r(_u(gen, N, H, W, Ci)), o["b_in"][0], o["b_in"][1])
    return o
