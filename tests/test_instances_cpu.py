"""CPU (no GPU needed): every template instantiation the conv kernels' host dispatchers can launch is either reached by a case of
tests/instance_cases.py or listed there as unreachable, with its arithmetic.

The instantiated sets are read from the dispatch macros in csrc/*.hip; the reachable sets come from sweeping the host-side queries
(mnas_conv_gemm_instance, mnas_tconv_dgrad_instance, mnas_conv_wgrad_instance, mnas_pw_bwd_instance, mnas_dw_geometry: each IS the
launch function stopped where it would launch) over channel counts in multiples of 8 up to 2048, the pixel-count classes on both
sides of every numeric gate, both modes and every pointer-presence form.  A new instantiation without a case, a case that no longer
maps to the instance it names, or a planner change that makes an instance (un)reachable fails here, before anything reaches a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import instance_cases as IC
from bounds_conv import act_interval, dy_interval
from bounds_se import gate_nhwc, gated_act_interval, sigmoid_interval
from mnasnet_pytorch_amd import _lib as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mnasnet_pytorch_amd", "csrc")


def _src(name):
    s = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", s)


def _entries(text, macro, n):
    """the integer argument tuples of every use of a dispatch macro (its #define has identifiers, not digits)"""
    return [tuple(int(v) for v in m) for m in re.findall(r"\b%s\(%s\)" % (macro, r",\s*".join([r"(\d+)"] * n)), text)]


def instantiated():
    """family -> set of instance tuples (as instance_cases names them), from the source text"""
    inst = {}
    pws = _src("mnas_pws.hip")
    assert "if constexpr (MODE == 0 && KSW <= 3)" in pws, "the gated instantiation rule of pws_launch changed: restate it here"
    e = _entries(pws, "MNAS_PWS", 3)
    inst["k_pws"] = {(m, nt, ksw, nw, 0) for m in (0, 1) for nt, ksw, nw in e} | {(0, nt, ksw, nw, 1) for nt, ksw, nw in e if ksw <= 3}
    pwf = _src("mnas_pwf.hip")
    assert "if (p.wres) hipLaunchKernelGGL((k_pwf<MODE, NT, PT, true>)" in pwf and "else if (MODE == 0) hipLaunchKernelGGL((k_pwf<0, NT, PT, false>)" in pwf
    inst["k_pwf"] = {(nt, pt, wres) for (nt,) in _entries(pwf, "MNAS_PWF", 1) for pt in (1, 2) for wres in (0, 1)}
    inst["k_pwd"] = {(nt, pt) for (nt,) in _entries(pwf, "MNAS_PWD", 1) for pt in (1, 2)}
    inst["k_pwx"] = set(_entries(_src("mnas_pwx.hip"), "MNAS_PWX", 3))
    inst["k_dimg"] = set(_entries(_src("mnas_dimg.hip"), "MNAS_DIMG", 3))
    c3r = _src("mnas_c3r.hip")
    assert "(k_c3r<M_, NT_, K_, 2>)" in c3r
    kq8 = {tuple(int(v) for v in m) for m in re.findall(r"k_c3r<(\d+), (\d+), (\d+), (\d+), (\d+)>", c3r)}
    inst["k_c3r"] = {(m, nt, k, 2, 4) for m, nt, k in _entries(c3r, "MNAS_C3R", 3)} | kq8
    inst["k_c3x"] = set(_entries(_src("mnas_c3x.hip"), "MNAS_C3X", 2))
    inst["k_igemm"] = {(m, nt, pt) for m, nt in _entries(_src("mnas_gemm.hip"), "MNAS_IG", 2) for pt in (1, 2)}
    tcx = _src("mnas_tcx.hip")
    inst["k_tcx"] = set(_entries(tcx, "MNAS_TCX", 2))
    inst["k_tcr"] = {tuple(int(v) for v in m) for m in re.findall(r"\(k_tcr<(\d+), (\d+), (\d+)>\)", tcx)}
    inst["k_tconv"] = {(nt, pt) for (nt,) in _entries(_src("mnas_tconv.hip"), "MNAS_TC", 1) for pt in (1, 2)}
    wg = _src("mnas_wgrad.hip")
    assert "#define MNAS_WTC(C_) MNAS_WT(C_, 1) MNAS_WT(C_, 2) MNAS_WT(C_, 3) MNAS_WT(C_, 4)" in wg
    inst["k_wgrad_t"] = set(_entries(wg, "MNAS_WT", 2)) | {(c, k) for (c,) in _entries(wg, "MNAS_WTC", 1) for k in (1, 2, 3, 4)}
    pwb = _src("mnas_pwbwd.hip")
    assert "if constexpr ((NTI > NTO && NTI >= 3) || (NTI == NTO && NTI >= 5))" in pwb and "if constexpr (NTO > NTI && NTI <= 2)" in pwb
    s = set()
    for nto, nti, pt in _entries(pwb, "MNAS_PWB", 3):
        s.add((nto, nti, pt, 0, 0))
        if (nti > nto and nti >= 3) or (nti == nto and nti >= 5):
            s.add((nto, nti, pt, 1, 0))
        if nto > nti and nti <= 2:
            s.add((nto, nti, pt, 0, 2))
    inst["k_pw_bwd"] = s
    dw = _src("mnas_dw.hip")
    inst["k_dw_fwd"] = set(_entries(dw, "MNAS_DWF", 2))
    assert "if (g == 4) MNAS_DWB(K_, DG_, WG_, R_, 4); else MNAS_DWB(K_, DG_, WG_, R_, 2);" in dw
    phase = {("true", "true"): 0, ("true", "false"): 1, ("false", "true"): 2}
    inst["k_dw_bwd"] = {(int(k), phase[(dg, wgf)], g) for k, dg, wgf, _ in
                        re.findall(r"MNAS_DWB_G\((\d), (true|false), (true|false), (true|false)\)", dw) for g in (2, 4)}
    return inst


def test_macro_tables_have_the_known_sizes():
    """the reader sees what the sources hold today (a regular expression that silently matches nothing would pass everything)"""
    sizes = {f: len(s) for f, s in instantiated().items()}
    assert sizes == {"k_pws": 32, "k_pwf": 24, "k_pwd": 12, "k_pwx": 3, "k_dimg": 8, "k_c3r": 8, "k_c3x": 2, "k_igemm": 24, "k_tcx": 2,
                     "k_tcr": 1, "k_tconv": 10, "k_wgrad_t": 19, "k_pw_bwd": 19, "k_dw_fwd": 4, "k_dw_bwd": 12}, sizes


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------
CH = range(8, 2049, 8)
# pixel counts (N, H, W) of the 1x1 launches: small; both sides of 250 000 (k_pwx, k_pws), of 400 000 (128-pixel tiles of k_pwf /
# k_pwd) and of 131 072 x cout blocks (k_igemm: one block at 131 072, two at 65 536, four at 32 768 ...)
PW_PIXELS = [(3, 11, 13), (250, 25, 40), (13, 601, 32), (39, 641, 16), (250, 40, 40), (8, 64, 64), (8, 64, 65), (16, 64, 64), (33, 63, 65),
             (32, 64, 64), (2, 64, 64), (4, 64, 64)]
PW_FORMS = {0: [dict(virt=True), dict(virt=False), dict(virt=True, gate=True), dict(virt=True, resid=True)],
            1: [dict(coef=True), dict(coef=False), dict(coef=True, resid=True), dict(coef=False, resid=True), dict(coef=True, red=True)]}
# 3x3: (N, H, W, stride) -- N on both sides of 32; output planes of <= 64 pixels (k_c3r; two images per pass in k_dimg), <= 128, <= 256
# and above; stride 2 onto them; the large maps on both sides of 100 000 output pixels (k_c3x)
D_PLANES = [(33, 3, 4, 1), (31, 3, 4, 1), (33, 6, 7, 1), (32, 8, 8, 1), (32, 9, 9, 1), (33, 12, 11, 1), (512, 12, 11, 1), (32, 16, 16, 1),
            (32, 17, 16, 1), (33, 5, 5, 2), (33, 23, 21, 2), (33, 16, 16, 2), (9, 221, 213, 2), (8, 221, 213, 2), (3, 11, 13, 1)]
D_FORMS = {0: [dict(virt=True), dict(virt=False)], 1: [dict(coef=False), dict(coef=False, red=True), dict(coef=True)]}


def _sweep_gemm():
    """reachable (family, instance) -> a witness spec, over the 1x1 and 3x3 launches of mnas_conv_gemm"""
    lib = L.load()
    out = (C.c_int * 8)()
    seen = {}
    fams = IC.ROUTES
    for mode in (0, 1):
        for k, shapes, forms in ((1, [s + (1,) for s in PW_PIXELS], PW_FORMS[mode]), (3, D_PLANES, D_FORMS[mode])):
            for form in forms:
                if k == 1 and len(form) > 1 or k == 3 and form.get("red"):
                    shp = shapes[:2] + shapes[4:5] + shapes[8:9] if k == 1 else shapes[:6]      # (the pointer forms do not move a numeric gate)
                else:
                    shp = shapes
                for (N, H, W, s) in shp:
                    a = IC.gemm_struct(mode, N, H, W, 8, 8, k, s, **form)
                    ref = C.byref(a)
                    big = N * H * W
                    for Ci in CH:
                        if k == 3 and (big * Ci > (1 << 31) or Ci > 1024 and mode == 0):
                            break
                        if mode == 0:
                            a.Ci = Ci
                        else:
                            a.Co = Ci
                        for Co in CH:
                            if mode == 0:
                                a.Co = Co
                            else:
                                a.Ci = Co
                            r = lib.mnas_conv_gemm_instance(ref, out)
                            if r < 0:
                                continue
                            fam = fams[r]
                            if fam == "k_igemm":
                                key = (fam, (mode, out[0], out[1]))
                            elif fam in ("k_pws", "k_c3r"):
                                key = (fam, (mode, out[0], out[1], out[2], out[3]))
                            elif fam == "k_dimg":
                                key = (fam, (mode, out[0], out[1]))
                            elif fam == "k_pwd" or fam == "k_c3x":
                                key = (fam, (out[0], out[1]))
                            else:
                                key = (fam, (out[0], out[1], out[2]))
                            if key not in seen:
                                seen[key] = (mode, N, H, W, Ci, Co, k, s, form)
    return seen


def _sweep_rest():
    lib = L.load()
    seen = {}
    for (N, Ho, Wo) in [(2, 9, 11), (3, 13, 9), (32, 7, 7), (33, 6, 7), (31, 7, 7), (8, 224, 224), (8, 223, 224), (2, 56, 56)]:
        for Co in CH:
            for Ci in CH:
                r = IC.tconv_instance_of(N, Ho, Wo, Co, Ci)
                if r is not None:
                    seen.setdefault(r[:2], (N, Ho, Wo, Co, Ci))
            if Co > 256 and Co != 192:
                break                                        # (every kernel refuses more than 256 dy channels)
    for k in (1, 3):
        for Co in CH:
            for Ci in (CH if k == 1 else range(8, 1025, 8)):
                r = IC.wgrad_instance_of(2, 7, 9, Ci, Co, k)
                seen.setdefault(r[:2], (2, 7, 9, Ci, Co, k))
    for Ci in CH:
        for Co in CH:
            if not lib.mnas_pw_bwd_supported(Ci, Co):
                continue
            for M in (429, 1 << 20):
                for red in (0, 1, 2):
                    for resid in (0, 1):
                        for recomp in (0, 1):
                            for masked in (0, 1):
                                r = IC.pw_bwd_instance_of(M, Ci, Co, red, resid, recomp, masked)
                                if r is not None:
                                    seen.setdefault(r[:2], (M, Ci, Co, red, resid, recomp, masked))
    for ks in (3, 5):
        for which in (0, 1, 2, 3):
            for C_ in CH:
                for H in (1, 7, 56):
                    for W in (4, 5, 7, 13, 14, 28, 56, 57, 112, 224, 512):
                        r = IC.dw_instance_of(2, H, W, C_, ks, which)
                        if r is not None:
                            seen.setdefault(r[:2], (2, H, W, C_))
    return seen


@pytest.fixture(scope="module")
def reachable():
    seen = _sweep_gemm()
    seen.update(_sweep_rest())
    return seen


def test_reachable_and_unreachable_partition_the_instantiated_set(reachable):
    inst = instantiated()
    table = {(f, i) for f, s in inst.items() for i in s}
    reach = set(reachable)
    dead = {(f, tuple(i)) for f, i, _ in IC.UNREACHABLE}
    assert len(dead) == len(IC.UNREACHABLE), "an instantiation is listed twice in UNREACHABLE"
    assert all(reason for _, _, reason in IC.UNREACHABLE)
    assert not (reach & dead), ("listed as unreachable, yet the sweep reaches it", sorted((k, reachable[k]) for k in reach & dead))
    assert reach - table == set(), ("the library launches an instance the macro reader does not know", sorted(reach - table))
    assert table - reach - dead == set(), ("instantiated, not reached by the sweep and not in UNREACHABLE", sorted(table - reach - dead))
    assert dead - table == set(), ("UNREACHABLE names an instantiation the sources do not have", sorted(dead - table))


def test_cases_map_to_their_instances_and_cover_the_reachable_set(reachable):
    named = set()
    for case in IC.CASES:
        family, inst, spec = case
        r = IC.instance_of(*case)
        assert r is not None, ("the launch of this case is refused", case)
        assert (r[0], r[1]) == (family, inst), ("case maps to another instance", case, r)
        named.add((family, inst))
    reach = set(reachable)
    assert reach - named == set(), ("reachable instantiation without a case (a witness each)", sorted((k, reachable[k]) for k in reach - named))
    assert named - reach == set(), ("a case names an instance the sweep does not reach: widen the sweep", sorted(named - reach))


def test_plan_values_that_pick_a_code_path_have_cases():
    """k_dimg with two images per pass and with several K chunks, k_pwf with resident and non-resident weights, k_c3r with several
    slices; PLAN_UNREACHABLE's entries hold for every case"""
    raw = {}
    for case in IC.CASES:
        raw.setdefault(case[0], []).append(IC.instance_of(*case)[2])
    for mode in (0, 1):
        d = [o for c, o in zip([c for c in IC.CASES if c[0] == "k_dimg"], raw["k_dimg"]) if c[1][0] == mode]
        assert any(o[2] > 1 for o in d) and any(o[2] == 1 for o in d), ("k_dimg mode %d: images per pass" % mode, d)
        assert any(o[3] > 1 for o in d) and any(o[3] == 1 for o in d), ("k_dimg mode %d: K chunks" % mode, d)
    assert {o[2] for o in raw["k_pwf"]} == {0, 1}
    assert all(o[3] == 1 for o in raw["k_pwf"] + raw["k_pwd"]), "k_pwf with several K chunks became reachable: add cases"
    assert all(o[4] > 1 for o in raw["k_c3r"])
    assert all(o[2] == 1 for o in raw["k_tcx"])


def test_findings_map_to_their_instances():
    for case in IC.FINDINGS:
        r = IC.instance_of(*case)
        assert r is not None and r[:2] == case[:2], (case, r)


def test_register_resident_slices_fit_their_instantiation():
    """the kernels that keep a weight slice in KSW (KS) fragments per wave: the plan never hands an instantiation more k-steps or
    cout tiles than its template arguments hold (k_c3r took 25..28 k-steps per wave on its 24-fragment instance before this test)"""
    cd = lambda a, b: (a + b - 1) // b
    n = 0
    for mode in (0, 1):
        for (N, H, W, k, s) in ((33, 3, 4, 3, 1), (33, 7, 7, 3, 1), (33, 13, 13, 3, 2), (3, 11, 13, 1, 1), (9, 221, 213, 3, 2)):
            if mode == 1 and s == 2:
                continue
            for Co in (8, 56, 104, 200, 320, 520):
                a = IC.gemm_struct(mode, N, H, W, 8, Co, k, s, **(dict(virt=True) if mode == 0 else dict(coef=(k == 1))))
                for K in CH:                       # K: the reduction's channels (struct Ci in either mode)
                    if k == 3 and (K > 1024 or N * H * W * K > (1 << 30)):
                        break
                    a.Ci = K
                    if mode == 1:
                        a.Co = Co
                    r = IC.gemm_instance_of(a)
                    if r is None:
                        continue
                    fam, inst, o = r
                    ksteps, tiles = cd(k * k * K, 32), cd(a.Co, 16)
                    if fam == "k_c3r":
                        assert cd(ksteps, o[3]) <= o[1] and o[0] * o[4] >= tiles, ("k_c3r", mode, (N, H, W), K, Co, o)
                    elif fam == "k_pws":
                        assert cd(ksteps, o[2]) <= o[1], ("k_pws", mode, K, Co, o)
                    elif fam == "k_pwx":
                        assert ksteps == o[1] and o[0] * o[2] * (1 if ksteps <= 3 else tiles // 24) >= tiles, ("k_pwx", K, Co, o)
                    elif fam == "k_c3x":
                        assert ksteps <= o[1] and tiles <= o[0], ("k_c3x", K, Co, o)
                    else:
                        continue
                    n += 1
    assert n > 500


def _tile_pixels(family, inst, raw):
    """pixels of the instance's tile along the dimension its grid walks"""
    if family in ("k_pws", "k_pwx", "k_c3x", "k_tcx"):
        return 16
    if family in ("k_pwf", "k_pwd", "k_tconv"):
        return 64 * inst[1]
    if family in ("k_igemm", "k_pw_bwd"):
        return 64 * inst[2]
    if family == "k_wgrad_t":
        return 64
    return 16            # the whole-image kernels: 16-pixel MFMA groups inside the plane(s) of a pass


@pytest.mark.parametrize("case", IC.CASES, ids=[IC.case_id(c) for c in IC.CASES])
def test_case_shape_is_ragged(case):
    """the pixel count is no multiple of the instance's pixel tile, and more than one tile; where the plan admits it the output
    channels leave the last 16-channel tile ragged"""
    family, inst, spec = case
    raw = IC.instance_of(*case)[2]
    if family in IC.ROUTES:
        mode, N, H, W, Ci, Co, k, s, form = spec
        p = k // 2
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        if family in ("k_dimg", "k_c3r"):
            plane = (Ho * Wo if mode == 0 else H * W) * (raw[2] if family == "k_dimg" else 1)
            assert plane % 16 != 0, (case, plane)
        else:
            M = N * Ho * Wo if mode == 0 else N * H * W
            t = _tile_pixels(family, inst, raw)
            assert M % t != 0 and M > t, (case, M, t)
        nout = Co if mode == 0 else Ci
        ragged_possible = not (family in ("k_pwf", "k_pwd") and inst[0] == 1)          # (one tile above 8 input channels: 16 outputs)
        assert nout % 16 == 8 or not ragged_possible, (case, nout)
    elif family in IC.TCONV_KERNELS:
        N, Ho, Wo, Co, Ci = spec
        if family != "k_tcr":
            assert (N * Ho * Wo) % _tile_pixels(family, inst, raw) != 0
        else:
            assert (Ho * Wo) % 16 != 0 and N % 2 == 1
    elif family in ("k_wgrad_t", "k_pw_bwd"):
        M = spec[0] * spec[1] * spec[2]
        t = _tile_pixels(family, inst, raw)
        assert M % t != 0 and M > t
        if family == "k_wgrad_t":
            assert spec[4] % 32 != 0 and spec[3] * spec[5] ** 2 % 32 != 0          # the slab's last cout and k tiles are ragged
    else:
        N, H, W, C_ = spec
        assert H % inst[-1] != 0 and W % 4 != 0


SMALL = [c for c in IC.CASES if c[0] in IC.ROUTES and IC.case_elements(c) < 1_000_000]


@pytest.mark.parametrize("case", SMALL, ids=[IC.case_id(c) for c in SMALL])
def test_small_case_operands_meet_the_helpers_conditions(case):
    """the operands the GPU test will launch with (built on the CPU from the case's seed): at most 1e-3 of the activation elements and
    2e-2 of the dy elements straddle a bf16 rounding boundary, at most 1 % were moved off the ReLU hinge (asserted inside
    off_hinge, act_interval, dy_interval and gated_act_interval)"""
    family, inst, spec = case
    mode, form = spec[0], spec[8]
    o = IC.gemm_operands(spec)             # off_hinge asserts its share
    if mode == 0 and form.get("gate"):
        iv = gated_act_interval(o["x"], o["sc"], o["sh"], gate_nhwc(sigmoid_interval(o["u"]), o["x"].shape), True)
        assert iv.split_share() <= 1e-3
    elif mode == 0 and form.get("virt", True):
        iv = act_interval(o["x"], o["sc"], o["sh"], True)
        assert iv.split_share() <= 1e-3
    elif mode == 1 and form.get("coef", True):
        iv = dy_interval(o["g"], o["y"], o["b"], True)
        assert iv.split_share() <= 2e-2
    if mode == 1 and form.get("red"):
        from bounds_conv import relu_mask
        relu_mask(o["y_in"], o["b_in"][0], o["b_in"][1])          # asserts: nothing left on the hinge
