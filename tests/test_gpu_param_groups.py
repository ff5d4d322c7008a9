"""-m gpu: parameter groups, decoupled weight decay and the LAMB / LARS trust ratios on the flat buffers (include/mnas.h:
mnas_*_step_seg; train_step.FlatAdam / FlatRMSprop / FlatSGD).  Oracles: the plain kernels themselves, launched once per parameter
tensor (bit for bit); torch's CPU optimizers with real param groups; the per-element brackets of tests/bounds_groups.py; the fp64
numpy reference tests/groups_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

import bounds_groups as BG
import bounds_tail as BT
import groups_ref as GR
from gpu_util import L, bits_equal, guarded
from intervals import check_interval
from test_gpu_gradclip import KINDS, _grads
from test_gpu_train import rl2

pytestmark = pytest.mark.gpu

HYPER = {"adam": BG.ADAM, "rmsprop": BG.RMSPROP, "sgd": BG.SGD}
BUFS = {"adam": ("p", "g", "m", "v"), "rmsprop": ("p", "g", "v", "buf"), "sgd": ("p", "g", "buf")}
TABLE = [2.25, 4.0, 0.0625]            # test_ex_kernels_per_element_bracket's partial table: the sum is exact, norm = sqrt(6.3125)
_CACHE = {}


def _layout(name):
    """(layout, tables, device tables, flat state): built once per layout and left unchanged"""
    from mnasnet_pytorch_amd.train_step import build_opt_tables
    if name not in _CACHE:
        lay = BG.standard_layout() if name == "standard" else BG.many_layout()
        tb = build_opt_tables(*lay)
        st = BG.trust_state(lay, tb) if name == "standard" else BG.flat_state(lay, 9)
        _CACHE[name] = (lay, tb, BG.tables_device(tb), st)
    return _CACHE[name]


def _device(st, names, offset):
    """guarded device copies of the flat state at element `offset` -> (buffers, canary checks)"""
    buf, chk = {}, {}
    for k in names:
        buf[k], chk[k] = guarded((st[k].numel(),), torch.float32, offset=offset)
        buf[k].copy_(st[k])
    return buf, chk


def _extra(mode, partial, stats, ema_ptr, table=None):
    if mode == "plain":
        return None
    return L.MnasOptExtra(partial=partial.data_ptr(), nparts=3, max_norm=0.9 if mode == "clip" else 1e3, skip_nonfinite=1,
                          ema=ema_ptr if mode == "ema" else None, ema_decay=0.999 if mode == "ema" else 0.0,
                          stats=stats.data_ptr(), update_stats=1)


def _plain_per_segment(kind, buf, a, groups, tb, ex):
    """mnas_<kind>_step (ex None) or _step_ex once per segment with the segment's group's lr and weight_decay"""
    lib = L.load()
    for k, (begin, n, gi) in enumerate(s[:3] for s in tb.segs):
        lr, wd = groups[gi][:2]
        P = lambda name: buf[name].data_ptr() + 4 * begin
        tail, sfx = [], ""
        if ex is not None:
            e = L.MnasOptExtra(partial=ex.partial, nparts=ex.nparts, max_norm=ex.max_norm, skip_nonfinite=ex.skip_nonfinite,
                               ema=ex.ema + 4 * begin if ex.ema else None, ema_decay=ex.ema_decay, stats=ex.stats,
                               update_stats=1 if k == 0 else 0)
            tail, sfx = [ctypes.byref(e)], "_ex"
        fn = getattr(lib, "mnas_%s_step%s" % (kind, sfx))
        if kind == "adam":
            rc = fn(P("p"), P("g"), P("m"), P("v"), n, lr, a["b1"], a["b2"], a["eps"], wd, a["step"], a["gscale"], *tail, L.cur_stream())
        elif kind == "rmsprop":
            rc = fn(P("p"), P("g"), P("v"), P("buf"), n, lr, a["alpha"], a["eps"], wd, a["momentum"], a["gscale"], *tail, L.cur_stream())
        else:
            rc = fn(P("p"), P("g"), P("buf"), n, lr, a["momentum"], a["dampening"], wd, a["nesterov"], a["step"], a["gscale"], *tail,
                    L.cur_stream())
        assert rc == 0, (kind, k, rc)


def _stats(t):
    raw = L.MnasGradStats()
    host = t.cpu()
    ctypes.memmove(ctypes.byref(raw), host.data_ptr(), 32)
    return raw


@pytest.mark.parametrize("layout", ["standard", "many"])
@pytest.mark.parametrize("mode", ["plain", "clip", "ema"])
@pytest.mark.parametrize("kind", ["adam", "rmsprop", "sgd"])
def test_groups_are_the_plain_kernels_bit_for_bit(kind, mode, layout):
    """ONE _seg call over three coupled groups == mnas_<kind>_step (extra NULL) / _step_ex (clipping active; EMA on) launched once per
    parameter tensor with that tensor's group's lr and weight_decay: p, both moments and the EMA bit for bit, g and the frozen tensor
    untouched, the stats block moved once, the canaries around the unaligned buffers intact.  Then a NaN table under skip_nonfinite:
    nothing moves but the counters."""
    lay, tb, dev, st = _layout(layout)
    a = HYPER[kind]
    names = BUFS[kind] + (("ema",) if mode == "ema" else ())
    groups = [g + (0, 0) for g in BG.GROUPS3]
    A, chk = _device(st, names, 1 if kind != "rmsprop" else 3)
    B, _ = _device(st, names, 3)
    partial = torch.tensor(TABLE, dtype=torch.float64, device="cuda")
    stats_a, stats_b = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2))
    ex_a = _extra(mode, partial, stats_a, A["ema"].data_ptr() if mode == "ema" else None)
    ex_b = _extra(mode, partial, stats_b, B["ema"].data_ptr() if mode == "ema" else None)
    assert BG.seg_call(kind, A, a, groups, tb, dev, ex=ex_a) == 0
    _plain_per_segment(kind, B, a, groups, tb, ex_b)
    what = "%s %s %s" % (kind, mode, layout)
    for k in names:
        chk[k](what + " " + k, written=False)
        bits_equal(A[k], B[k], what + " " + k)
    bits_equal(A["g"], st["g"].cuda(), what + " g")
    assert not torch.equal(A["p"].cpu(), st["p"])
    for (lo, hi), rg in zip(lay[0], lay[1]):
        if not rg:
            for k in names:
                bits_equal(A[k][lo:hi], st[k][lo:hi].cuda(), what + " frozen " + k)
    if mode == "plain":
        return
    sa, sb = _stats(stats_a), _stats(stats_b)
    assert sa.steps == 1 and (sa.last_norm, sa.last_coef, sa.clipped_steps, sa.skipped_steps) == \
        (sb.last_norm, sb.last_coef, sb.clipped_steps, sb.skipped_steps) and sa.clipped_steps == int(mode == "clip")
    # a NaN table under skip_nonfinite: every buffer bitwise untouched
    before = {k: v.clone() for k, v in A.items()}
    partial.copy_(torch.tensor([2.25, float("nan"), 0.0625], dtype=torch.float64))
    assert BG.seg_call(kind, A, a, groups, tb, dev, ex=ex_a) == 0
    for k in names:
        bits_equal(A[k], before[k], what + " skipped step, " + k)
        chk[k](what + " skipped " + k, written=False)
    sa = _stats(stats_a)
    assert sa.steps == 2 and sa.skipped_steps == 1


def _views(flat, sizes):
    out, off = [], 0
    for k in sizes:
        par = torch.nn.Parameter(flat[off:off + k])
        par.data = flat[off:off + k]
        out.append(par)
        off += k
    return out


SPLIT = ([3000, 7, 4000, 1000, 2000], [0, 1, 2, 1, 0])           # five tensors of _grads()' 10007 elements over three groups
GROUP_KW = [dict(lr=1e-2, weight_decay=1e-2), dict(lr=3e-2, weight_decay=0.0), dict(lr=2e-3, weight_decay=5e-2)]


def _group_list(params):
    return [dict(GROUP_KW[k], params=[p for p, g in zip(params, SPLIT[1]) if g == k]) for k in range(3)]


@pytest.mark.parametrize("kind,kw", KINDS + [("adamw", {})])
def test_param_groups_match_torch(kind, kw):
    """_grads()' five steps, three groups with their own lr and weight_decay, a MultiStepLR stepped in between on both sides:
    FlatAdam / FlatRMSprop / FlatSGD against torch.optim.Adam / RMSprop / SGD on the CPU, decoupled_weight_decay=True against
    torch.optim.AdamW; rl2 < 1e-6 as in test_clipped_optimizers_match_torch."""
    from mnasnet_pytorch_amd.train_step import FlatAdam, FlatRMSprop, FlatSGD
    p0, grads = _grads()
    flat_p, flat_g = p0.clone().cuda(), torch.zeros(p0.numel(), device="cuda")
    fcls = {"adam": FlatAdam, "adamw": FlatAdam, "rmsprop": FlatRMSprop, "sgd": FlatSGD}[kind]
    tcls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}[kind]
    extra = {"decoupled_weight_decay": True} if kind == "adamw" else {}
    opt = fcls(_group_list(_views(flat_p, SPLIT[0])), flat_p, flat_g, lr=1.0, **kw, **extra)
    ref_flat = p0.clone()
    ref_params = _views(ref_flat, SPLIT[0])
    opt_ref = tcls(_group_list(ref_params), lr=1.0, **kw)
    scheds = [torch.optim.lr_scheduler.MultiStepLR(o, milestones=[2, 4], gamma=0.5) for o in (opt, opt_ref)]
    for g in grads:
        for par, gv in zip(ref_params, _views(g.clone(), SPLIT[0])):
            par.grad = gv.data.clone()
        opt_ref.step()
        flat_g.copy_(g.cuda())
        opt.step()
        for s in scheds:
            s.step()
    assert opt.seg_calls == 5
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in opt_ref.param_groups]
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([k["lr"] * 0.25 for k in GROUP_KW], rel=1e-12)
    err = rl2(flat_p.cpu(), ref_flat)
    print(kind, kw, "rl2 vs torch %.3g" % err)
    assert err < 1e-6, (kind, kw)


@pytest.mark.parametrize("mode", ["plain", "clip"])
@pytest.mark.parametrize("kind", ["adam", "rmsprop", "sgd"])
def test_decoupled_decay_per_element_bracket(kind, mode):
    """Groups 0 and 1 decoupled (one with weight_decay 0: f == 1), group 2 coupled, in ONE call; every output of every tensor inside
    bounds_groups.decoupled_intervals (bounds_tail's own bracket for the coupled group): worst error / bracket <= 1."""
    lay, tb, dev, st = _layout("standard")
    a = HYPER[kind]
    groups = [BG.GROUPS3[0] + (1, 0), BG.GROUPS3[1] + (1, 0), BG.GROUPS3[2] + (0, 0)]
    A, chk = _device(st, BUFS[kind], 3)
    partial = torch.tensor(TABLE, dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    ex = _extra(mode, partial, stats, None)
    assert BG.seg_call(kind, A, a, groups, tb, dev, ex=ex) == 0
    coef = BT.opt_coef_interval(TABLE, 0.9, st["p"])[2] if mode == "clip" else None
    out = {k: A[k].cpu() for k in BUFS[kind]}
    worst = 0.0
    for (begin, n, gi) in (s[:3] for s in tb.segs):
        s = BG.slice_state(st, begin, begin + n)
        lr, wd, dec, _ = groups[gi]
        if dec:
            ivs = BG.decoupled_intervals(kind, s, a, lr, wd, coef)
        elif kind == "adam":
            ivs = BT.adam_intervals(s["p"], s["g"], s["m"], s["v"], lr=lr, wd=wd, coef=coef, **a)
        elif kind == "rmsprop":
            ivs = BT.rmsprop_intervals(s["p"], s["g"], s["v"], s["buf"], lr=lr, wd=wd, coef=coef, **a)
            ivs["v"] = ivs.pop("sq")
        else:
            ivs = BT.sgd_intervals(s["p"], s["g"], s["buf"], lr=lr, wd=wd, coef=coef, **a)
        for k, iv in ivs.items():
            worst = max(worst, check_interval(out[k][begin:begin + n], iv, "%s decoupled %s segment at %d %s" % (kind, mode, begin, k),
                                              "optimizers, groups"))
    for k in BUFS[kind]:
        chk[k]("%s decoupled %s" % (kind, k), written=False)
    bits_equal(A["g"], st["g"].cuda(), "g")
    print("%s decoupled %s: worst error / bracket %.3f" % (kind, mode, worst))
    assert worst <= 1.0


TRUST_MODES = [("standard", "plain"), ("standard", "clip"), ("standard", "ema"), ("many", "plain")]


def _trust_run(kind, name, st, sentinel=-7.0, ema=False):
    lay, tb, dev, _ = _layout(name)
    A, chk = _device(st, BUFS[kind] + (("ema",) if ema else ()), 1)
    tpart = torch.full((2 * len(tb.tiles) + 2,), sentinel, dtype=torch.float64, device="cuda")
    ratio = torch.full((len(tb.segs) + 1,), sentinel, dtype=torch.float32, device="cuda")
    return lay, tb, dev, A, chk, tpart, ratio


def _trust_extra(mode, A):
    """-> (MnasOptExtra or None, stats block, partial table (kept alive), Interval of coef or None): 'clip' = coef < 1, no EMA;
    'ema' = the table present, coef == 1, the EMA behind the update"""
    if mode == "plain":
        return None, None, None, None
    partial = torch.tensor(TABLE, dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    ex = _extra(mode, partial, stats, A["ema"].data_ptr() if mode == "ema" else None)
    return ex, stats, partial, BT.opt_coef_interval(TABLE, ex.max_norm, torch.zeros(1))[2]


def _consumed_gradient(st, a, stats):
    """gs as the device forms it, in fp32: g gscale, then times the coefficient the step's stats block reports (exact data, read
    back like the ratios)"""
    gs = st["g"] * torch.tensor(a["gscale"])
    if stats is not None:
        sk = _stats(stats)
        assert sk.steps == 1 and sk.skipped_steps == 0
        gs = gs * torch.tensor(sk.last_coef, dtype=torch.float32)
    return gs.numpy()


def _seg_roots(tb, tpart):
    """per segment (float32 sqrt of the sum of its tiles' first partials, the same for the second): the finalize's inputs"""
    t = tpart.cpu().numpy()
    out = []
    for (_, _, _, t0, nt, _) in tb.segs:
        sw, s2 = 0.0, 0.0
        for k in range(t0, t0 + nt):
            sw, s2 = sw + t[2 * k], s2 + t[2 * k + 1]
        out.append((np.float32(np.sqrt(max(sw, 0.0))), np.float32(np.sqrt(max(s2, 0.0)))))      # (sentinels: tensors without a norm)
    return out


TRUST_GROUPS = [BG.GROUPS3[0] + (0, 1), BG.GROUPS3[1] + (0, 1), BG.GROUPS3[2] + (0, 0)]        # group 2: trust = False


@pytest.mark.parametrize("name,mode", TRUST_MODES)
def test_lamb_trust_ratios(name, mode):
    """One LAMB call with extra NULL, with the clip active (coef < 1: the norm pass and the update must both consume
    (g gscale) coef) and with the EMA behind the update.  w against groups_ref to 2^-23; un and r inside the hull of bounds_groups; p, m, v inside their per-element
    brackets with r read back; an all-zero weight tensor, a tensor with u == 0 and the trust = False group have r == 1.0 exactly;
    the slot behind the last segment (and the frozen tensor) untouched; a second run from the same state gives the same bits; a NaN
    table under skip_nonfinite writes neither the buffers nor the workspaces."""
    _, _, _, st = _layout(name)
    lay, tb, dev, A, chk, tpart, ratio = _trust_run("adam", name, st, ema=mode == "ema")
    a = BG.ADAM
    ex, stats, _partial, coef = _trust_extra(mode, A)
    assert BG.seg_call("adam", A, a, TRUST_GROUPS, tb, dev, trust_kind=L.TRUST_LAMB, ws=(tpart, ratio), ex=ex) == 0
    r_dev = ratio.cpu().numpy()
    roots = _seg_roots(tb, tpart)
    tp = tpart.cpu()
    assert r_dev[-1] == -7.0 and float(tp[-1]) == -7.0
    out = {k: A[k].cpu() for k in BUFS["adam"]}
    gs = _consumed_gradient(st, a, stats)
    if mode == "clip":
        assert _stats(stats).last_coef < 0.5 and _stats(stats).clipped_steps == 1
    worst, real = 0.0, 0
    for k, (begin, n, gi, t0, nt, _) in enumerate(tb.segs):
        s = BG.slice_state(st, begin, begin + n)
        lr, wd, _, trust = TRUST_GROUPS[gi]
        if not trust:
            assert r_dev[k] == 1.0 and float(tp[2 * t0]) == -7.0               # no norm is taken of a trust = False tensor
        else:
            u_ref, _, _ = GR.lamb_direction(s["p"].numpy(), gs[begin:begin + n], s["m"].numpy(), s["v"].numpy(), a["b1"], a["b2"],
                                            a["eps"], wd, a["step"])
            w_ref, un_ref = GR.norm(s["p"].numpy()), GR.norm(u_ref)
            w_dev, un_dev = roots[k]
            assert abs(float(w_dev) - w_ref) <= 2.0 ** -23 * w_ref, (k, w_dev, w_ref)
            if w_ref == 0.0 or un_ref == 0.0:
                assert r_dev[k] == 1.0, (k, r_dev[k])
                assert (name == "many") or k in (BG.ZERO_P_SEG, BG.ZERO_G_SEG)
            else:
                u_iv = BG.lamb_direction(s, a, wd, coef)[0]
                un_lo, un_hi, r_lo, r_hi = BG.lamb_ratio_hull(w_ref, u_iv)
                assert un_lo <= float(un_dev) <= un_hi, (k, un_lo, float(un_dev), un_hi)
                assert r_lo <= float(r_dev[k]) <= r_hi, (k, r_lo, float(r_dev[k]), r_hi)
                real += 1
        if name == "standard":
            ivs = BG.lamb_intervals(s, a, lr, wd, r_dev[k], coef)
            for key, iv in ivs.items():
                worst = max(worst, check_interval(out[key][begin:begin + n], iv, "lamb segment %d %s" % (k, key), "optimizers, groups"))
    assert real >= 4
    if name == "standard":
        assert r_dev[BG.ZERO_P_SEG] == 1.0 and r_dev[BG.ZERO_G_SEG] == 1.0
        lo, hi = lay[0][BG.FROZEN_AT]
        for key in BUFS["adam"]:
            bits_equal(A[key][lo:hi], st[key][lo:hi].cuda(), "frozen " + key)
    for key in BUFS["adam"]:
        chk[key]("lamb " + key, written=False)
    bits_equal(A["g"], st["g"].cuda(), "g")
    if mode == "ema":
        chk["ema"]("lamb ema", written=False)
        worst = max(worst, BT.check_ema(A["ema"][:lo], 0.999, st["ema"][:lo], A["p"][:lo], "lamb ema, front", "optimizers, groups"),
                    BT.check_ema(A["ema"][hi:], 0.999, st["ema"][hi:], A["p"][hi:], "lamb ema, back", "optimizers, groups"))
        bits_equal(A["ema"][lo:hi], st["ema"][lo:hi].cuda(), "frozen ema")
    print("lamb %s %s: %d ratios inside their hulls, worst error / bracket %.3f" % (name, mode, real, worst))
    assert worst <= 1.0
    if mode != "plain":
        return
    # the same state again: the same bits
    _, _, _, B, _, tpart2, ratio2 = _trust_run("adam", name, st)
    assert BG.seg_call("adam", B, a, TRUST_GROUPS, tb, dev, trust_kind=L.TRUST_LAMB, ws=(tpart2, ratio2)) == 0
    bits_equal(ratio2, ratio, "ratio, second run")
    for key in ("p", "m", "v"):
        bits_equal(B[key], A[key], key + ", second run")
    # a skipped step writes nothing but the stats block
    partial = torch.tensor([2.25, float("inf"), 0.0625], dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    ex = _extra("clip", partial, stats, None)
    before = {key: v.clone() for key, v in B.items()}
    tpart2.fill_(-3.0)
    ratio2.fill_(-3.0)
    assert BG.seg_call("adam", B, a, TRUST_GROUPS, tb, dev, trust_kind=L.TRUST_LAMB, ws=(tpart2, ratio2), ex=ex) == 0
    for key in BUFS["adam"]:
        bits_equal(B[key], before[key], "skipped step, " + key)
    assert bool((tpart2 == -3.0).all()) and bool((ratio2 == -3.0).all())
    sk = _stats(stats)
    assert sk.steps == 1 and sk.skipped_steps == 1


@pytest.mark.parametrize("name,mode", TRUST_MODES)
def test_lars_trust_ratios(name, mode):
    """One LARS call with extra NULL, with the clip active (gn is the norm of (g gscale) coef) and with the EMA: w and gn against groups_ref to 2^-23, r to bounds_groups.LARS_RATIO_REL;
    p and the momentum buffer inside their brackets with r read back; the rules and the second run as for LAMB."""
    _, _, _, st = _layout(name)
    lay, tb, dev, A, chk, tpart, ratio = _trust_run("sgd", name, st, ema=mode == "ema")
    a, coef_c, eps_c = BG.SGD, 1e-3, 1e-8
    ex, stats, _partial, coef = _trust_extra(mode, A)
    assert BG.seg_call("sgd", A, a, TRUST_GROUPS, tb, dev, trust_kind=L.TRUST_LARS, trust_coef=coef_c, trust_eps=eps_c, ws=(tpart, ratio),
                       ex=ex) == 0
    r_dev = ratio.cpu().numpy()
    roots = _seg_roots(tb, tpart)
    assert r_dev[-1] == -7.0
    out = {k: A[k].cpu() for k in BUFS["sgd"]}
    gs = _consumed_gradient(st, a, stats)
    if mode == "clip":
        assert _stats(stats).last_coef < 0.5 and _stats(stats).clipped_steps == 1
    worst, real = 0.0, 0
    for k, (begin, n, gi, t0, nt, _) in enumerate(tb.segs):
        s = BG.slice_state(st, begin, begin + n)
        lr, wd, _, trust = TRUST_GROUPS[gi]
        if not trust:
            assert r_dev[k] == 1.0
        else:
            w_ref, gn_ref = GR.norm(s["p"].numpy()), GR.norm(gs[begin:begin + n])
            w_dev, gn_dev = roots[k]
            assert abs(float(w_dev) - w_ref) <= 2.0 ** -23 * w_ref and abs(float(gn_dev) - gn_ref) <= 2.0 ** -23 * gn_ref, k
            r_ref = GR.lars_ratio(w_ref, gn_ref, float(np.float32(wd)), float(np.float32(coef_c)), float(np.float32(eps_c)))
            if w_ref == 0.0 or gn_ref == 0.0:
                assert r_dev[k] == 1.0 and r_ref == 1.0
            else:
                assert abs(float(r_dev[k]) - r_ref) <= BG.LARS_RATIO_REL * r_ref, (k, float(r_dev[k]), r_ref)
                real += 1
        if name == "standard":
            ivs = BG.lars_intervals(s, a, lr, wd, r_dev[k], coef)
            for key, iv in ivs.items():
                worst = max(worst, check_interval(out[key][begin:begin + n], iv, "lars segment %d %s" % (k, key), "optimizers, groups"))
    assert real >= 3            # (standard: tensors 1, 6, 7; the one-element tensor 0 has g == 0, opt_data's every 11th element)
    if name == "standard":
        assert r_dev[BG.ZERO_P_SEG] == 1.0 and r_dev[BG.ZERO_G_SEG] == 1.0 and r_dev[0] == 1.0
        lo, hi = lay[0][BG.FROZEN_AT]
        for key in BUFS["sgd"]:
            bits_equal(A[key][lo:hi], st[key][lo:hi].cuda(), "frozen " + key)
    for key in BUFS["sgd"]:
        chk[key]("lars " + key, written=False)
    bits_equal(A["g"], st["g"].cuda(), "g")
    if mode == "ema":
        chk["ema"]("lars ema", written=False)
        worst = max(worst, BT.check_ema(A["ema"][:lo], 0.999, st["ema"][:lo], A["p"][:lo], "lars ema, front", "optimizers, groups"),
                    BT.check_ema(A["ema"][hi:], 0.999, st["ema"][hi:], A["p"][hi:], "lars ema, back", "optimizers, groups"))
        bits_equal(A["ema"][lo:hi], st["ema"][lo:hi].cuda(), "frozen ema")
    print("lars %s %s: %d ratios within 2^-21, worst error / bracket %.3f" % (name, mode, real, worst))
    assert worst <= 1.0
    if mode != "plain":
        return
    _, _, _, B, _, tpart2, ratio2 = _trust_run("sgd", name, st)
    assert BG.seg_call("sgd", B, a, TRUST_GROUPS, tb, dev, trust_kind=L.TRUST_LARS, trust_coef=coef_c, trust_eps=eps_c, ws=(tpart2, ratio2)) == 0
    bits_equal(ratio2, ratio, "ratio, second run")
    for key in ("p", "buf"):
        bits_equal(B[key], A[key], key + ", second run")
    # a skipped step writes nothing but the stats block
    partial = torch.tensor([2.25, float("nan"), 0.0625], dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    ex = _extra("clip", partial, stats, None)
    before = {key: v.clone() for key, v in B.items()}
    tpart2.fill_(-3.0)
    ratio2.fill_(-3.0)
    assert BG.seg_call("sgd", B, a, TRUST_GROUPS, tb, dev, trust_kind=L.TRUST_LARS, trust_coef=coef_c, trust_eps=eps_c, ws=(tpart2, ratio2),
                       ex=ex) == 0
    for key in BUFS["sgd"]:
        bits_equal(B[key], before[key], "skipped step, " + key)
    assert bool((tpart2 == -3.0).all()) and bool((ratio2 == -3.0).all())
    sk = _stats(stats)
    assert sk.steps == 1 and sk.skipped_steps == 1


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_optimizer_trust_ratio_surface(kind):
    """FlatAdam(trust_ratio='lamb') / FlatSGD(trust_ratio='lars') over real groups with a frozen tensor: trust_ratios() names the
    trainable tensors by index, the trust = False group reads 1.0, freezing another tensor rebuilds the tables, the parameters follow
    groups_ref over two steps (fp64 reference of fp32 arithmetic: 1e-5 relative L2 leaves three decimal orders over the fp32 unit
    roundoff for the ratio's amplification of a tensor-wide rounding difference)."""
    from mnasnet_pytorch_amd.train_step import FlatAdam, FlatSGD
    sizes, gidx = [300, 5, 4097, 64, 700], [0, 1, 0, 1, 0]
    gen = torch.Generator().manual_seed(21)
    n = sum(sizes)
    p0 = torch.randn(n, generator=gen)
    flat_p, flat_g = p0.clone().cuda(), torch.zeros(n, device="cuda")
    params = _views(flat_p, sizes)
    params[3].requires_grad_(False)
    glist = [{"params": [params[0], params[2], params[4]], "lr": 1e-2, "weight_decay": 1e-2},
             {"params": [params[1], params[3]], "lr": 2e-2, "weight_decay": 0.0, "trust": False}]
    if kind == "lamb":
        opt = FlatAdam(glist, flat_p, flat_g, trust_ratio="lamb")
    else:
        opt = FlatSGD(glist, flat_p, flat_g, momentum=0.9, trust_ratio="lars", trust_coef=0.02)
    assert opt.trust_ratios() is not None
    segs, off = [], 0
    for k, g in zip(sizes, gidx):
        segs.append((off, off + k, g))
        off += k
    ref_groups = [dict(lr=1e-2, wd=1e-2, trust=True), dict(lr=2e-2, wd=0.0, trust=False)]
    p, m, v = p0.numpy().astype(np.float64), np.zeros(n), np.zeros(n)
    for step in (1, 2):
        g = torch.randn(n, generator=gen)
        flat_g.copy_(g.cuda())
        opt.step()
        live = [(a, b, gi if i != 3 else None) for i, (a, b, gi) in enumerate(segs)]
        if kind == "lamb":
            p, m, v, info = GR.lamb_step(p, g.numpy(), m, v, live, ref_groups, 0.9, 0.999, 1e-8, step)
        else:
            p, m, info = GR.lars_step(p, g.numpy(), m, live, ref_groups, 0.9, 0.0, False, step == 1, 0.02, 1e-8)
        got = opt.trust_ratios()
        assert sorted(got) == [0, 1, 2, 4] and got[1] == 1.0
        for i in (0, 2, 4):
            assert abs(got[i] - info[i][2]) <= 1e-5 * info[i][2], (step, i, got[i], info[i][2])
        assert opt.last_trust_ratios.is_cuda and opt.last_trust_ratios.numel() == 4
    assert rl2(flat_p.cpu(), p) < 1e-5 and opt.seg_calls == 2
    assert torch.equal(flat_p[segs[3][0]:segs[3][1]].cpu(), p0[segs[3][0]:segs[3][1]])
    params[1].requires_grad_(False)                       # a changed requires_grad pattern: the tables follow
    opt.step()
    assert sorted(opt.trust_ratios()) == [0, 2, 4]
