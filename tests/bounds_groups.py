"""Per-element bounds and test layouts for the grouped optimizer steps (include/mnas.h: mnas_*_step_seg; csrc/mnas_elementwise.hip:
k_seg_step, k_seg_norm, k_seg_ratio).  Conventions of intervals.py; the coupled update's brackets are bounds_tail's own.

Decoupled decay.  The device multiplies p by f = (float)(1.0 - (double)lr (double)wd): the fp64 value 1 - lr wd of the fp32 scalars,
rounded ONCE to fp32 (the fp64 product and difference err by 2^-53, carried as D64), then p' = fl(p f): one more rounding.  The
optimizer's update then runs from p' with the undecayed gradient, bracketed operation by operation as in bounds_tail.

Trust ratios.  w = (float)sqrt(sum (double)p^2) and gn = (float)sqrt(sum (double)gs^2): the squares of fp32 values are exact in fp64,
the fp64 sum of n <= 2^24 non-negative terms errs by at most n 2^-53 relative, the root by 2^-53, the rounding to fp32 by 2^-24: the
tests hold both to 2^-23 of the reference.  un = (float)sqrt(sum (double)u^2) with u the device's own fp32 u[i], which the host does
not re-enact: u[i] lies in its per-element bracket [lo_i, hi_i] (lamb_direction), so |u[i]| lies in [a_i, b_i] with a_i = 0 where the
bracket holds 0, else min(|lo_i|, |hi_i|), and b_i = max(|lo_i|, |hi_i|); the sum of squares is monotone in every |u[i]|, hence
    sqrt(sum a_i^2) <= sqrt(sum (double)u[i]^2) <= sqrt(sum b_i^2)
and un, one fp32 rounding of that root (2^-24; the fp64 work is below 2^-40), lies in that hull widened by 2^-24.  r = fl(w / un)
with w within 2^-24 (one rounding) of the exact root W: r in [W / un_hi, W / un_lo] up to three factors (1 + 2^-24) -- w's
rounding, un's rounding, the division's -- i.e. widened by 3 2^-24 < 2^-22 relative, which is what lamb_ratio_hull applies.  LARS:
r = fl(fl(c w) / fl(fma(wd, w, gn) + eps)): w and gn each within 2^-23 of the reference, then four roundings (product, fma, sum,
quotient); every term of the denominator is non-negative, so relative errors do not amplify: |r - r_ref| <= (2 2^-23 + 4 2^-24)
r_ref = 2^-21 r_ref, lars_ratio_bound.  The update itself is bracketed with r READ BACK from the device table (exact data)."""
import ctypes as C

import torch

import bounds_tail as BT
from gpu_util import L
from intervals import D64, Interval, f32, widen

exact = Interval.exact
TILE = 4096

# ---- layouts (pure host data) -----------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 255, 257, 4095, 4096, 4097, 2 * 4096 + 300]       # around the wave, the workgroup and the tile; a 3-tile tensor
FROZEN_AT, FROZEN_N = 5, 8547                                         # one frozen tensor in the middle: 29967 elements in all


def standard_layout():
    """-> (ranges, requires_grad, group_index): the nine trainable tensors, groups 0, 1, 2, 0, 1, 2, ... in order (weight, bias,
    weight, bias, ... over three groups), the frozen tensor in front of the sixth"""
    sizes = SIZES[:FROZEN_AT] + [FROZEN_N] + SIZES[FROZEN_AT:]
    ranges, rg, gi, off, k = [], [], [], 0, 0
    for i, n in enumerate(sizes):
        ranges.append((off, off + n))
        off += n
        frozen = i == FROZEN_AT
        rg.append(not frozen)
        gi.append(0 if frozen else k % 3)
        k += 0 if frozen else 1
    return ranges, rg, gi


def many_layout(nseg=2100, n=5):
    """more tiles than the grid has workgroups (2048): every workgroup of the cap takes a second tile"""
    return [(i * n, (i + 1) * n) for i in range(nseg)], [True] * nseg, [i % 3 for i in range(nseg)]


def segments_of(layout):
    """groups_ref's (begin, end, group or None) list"""
    return [(a, b, g if rg else None) for (a, b), rg, g in zip(*layout)]


# ---- the C call ---------------------------------------------------------------------------------------------------------------------------
def tables_device(tb):
    def up(cls, rows):
        arr = (cls * max(1, len(rows)))(*[cls(*r) for r in rows])
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return up(L.MnasOptSeg, [s[:5] + (0,) for s in tb.segs]), up(L.MnasOptTile, tb.tiles)


def seg_call(kind, buf, a, groups, tb, dev_tables, trust_kind=0, trust_coef=1e-3, trust_eps=1e-8, ex=None, ws=None):
    """ONE mnas_<kind>_step_seg call.  buf: name -> device tensor whose element 0 is element 0 of the flat buffers (p, g, m, v, buf as
    in bounds_tail.opt_data); a: the optimizer's scalars (bounds_tail's names); groups: [(lr, wd, decoupled, trust)]; ws: (tile_partial,
    ratio) device tensors for a trust-ratio step; ex: a MnasOptExtra or None.  -> the return code"""
    lib = L.load()
    garr = (L.MnasOptGroup * len(groups))(*[L.MnasOptGroup(*g) for g in groups])
    s = L.MnasOptSegs(segs=dev_tables[0].data_ptr(), tiles=dev_tables[1].data_ptr(), groups=garr, nsegs=len(tb.segs), ntiles=len(tb.tiles),
                      ngroups=len(groups), trust_kind=trust_kind, tile_partial=ws[0].data_ptr() if ws else None,
                      ratio=ws[1].data_ptr() if ws else None, trust_coef=trust_coef, trust_eps=trust_eps)
    P = lambda k: buf[k].data_ptr()
    e = C.byref(ex) if ex is not None else None
    if kind == "adam":
        return lib.mnas_adam_step_seg(P("p"), P("g"), P("m"), P("v"), a["b1"], a["b2"], a["eps"], a["step"], a["gscale"], C.byref(s), e,
                                      L.cur_stream())
    if kind == "rmsprop":
        return lib.mnas_rmsprop_step_seg(P("p"), P("g"), P("v"), P("buf"), a["alpha"], a["eps"], a["momentum"], a["gscale"], C.byref(s), e,
                                         L.cur_stream())
    return lib.mnas_sgd_step_seg(P("p"), P("g"), P("buf"), a["momentum"], a["dampening"], a["nesterov"], a["step"], a["gscale"],
                                 C.byref(s), e, L.cur_stream())


# ---- brackets -----------------------------------------------------------------------------------------------------------------------------
def decay_interval(lr, wd):
    """f = (float)(1.0 - (double)lr (double)wd): one fp32 rounding of the fp64 value"""
    t = torch.tensor(1.0 - f32(lr) * f32(wd), dtype=torch.float64)
    return Interval(*widen(t, t, 1, host=D64))


def _update(kind, pi, gi, st, a, lr):
    """the three updates of bounds_tail (same operations, same roundings) from an Interval pi of the weight the update starts from and
    an Interval gi of the gradient it consumes; st: the fp32 state tensors"""
    like = st["g"]
    s = lambda c: exact(c, like=like)
    lr = f32(lr)
    if kind == "adam":
        b1, b2, eps = f32(a["b1"]), f32(a["b2"]), f32(a["eps"])
        bc1, bc2s = BT.adam_bias(b1, b2, a["step"])
        step_size = float(torch.tensor(lr, dtype=torch.float32) / torch.tensor(bc1, dtype=torch.float32))
        mi = s(b1).fma(exact(st["m"]), s(BT._om(b1)).mul(gi, 1))
        vi = s(b2).fma(exact(st["v"]), s(BT._om(b2)).mul(gi, 1).mul(gi, 1))
        vi = Interval(vi.lo.clamp_min(0.0), vi.hi)
        den = vi.sqrt().div(s(bc2s), 1).add(s(eps), 1)
        return dict(p=pi.add(s(step_size).mul(mi.div(den, 1), 1), 1, -1.0), m=mi, v=vi)
    if kind == "rmsprop":
        alpha, eps, momentum = f32(a["alpha"]), f32(a["eps"]), f32(a["momentum"])
        si = s(alpha).fma(exact(st["v"]), s(BT._om(alpha)).mul(gi, 1).mul(gi, 1))
        si = Interval(si.lo.clamp_min(0.0), si.hi)
        r = gi.div(si.sqrt().add(s(eps), 1), 1)
        out = dict(v=si)
        if momentum > 0:
            r = s(momentum).fma(exact(st["buf"]), r)
            out["buf"] = r
        out["p"] = pi.add(s(lr).mul(r, 1), 1, -1.0)
        return out
    momentum, dampening = f32(a["momentum"]), f32(a["dampening"])
    out = {}
    if momentum != 0.0:
        b = gi if a["step"] == 1 else s(momentum).fma(exact(st["buf"]), s(BT._om(dampening)).mul(gi, 1))
        out["buf"] = b
        gi = s(momentum).fma(b, gi) if a["nesterov"] else b
    out["p"] = pi.add(s(lr).mul(gi, 1), 1, -1.0)
    return out


def decoupled_intervals(kind, st, a, lr, wd, coef=None):
    """p' = fl(p f) (decay_interval), then the optimizer's update of p' from gs without decay"""
    pi = exact(st["p"]).mul(decay_interval(lr, wd), 1)
    gi = BT._opt_grad(st["p"], st["g"], 0.0, a["gscale"], coef)
    return _update(kind, pi, gi, st, a, lr)


def lamb_direction(st, a, wd, coef=None):
    """(u, m', v') Intervals: m, v from gs without decay; u = fl(fl(m / bc1) / denom), wd != 0: fl(fl(wd p) + u) -- two roundings, of
    which a fused multiply-add takes one (a superset)"""
    like = st["g"]
    s = lambda c: exact(c, like=like)
    b1, b2, eps = f32(a["b1"]), f32(a["b2"]), f32(a["eps"])
    bc1, bc2s = BT.adam_bias(b1, b2, a["step"])
    gi = BT._opt_grad(st["p"], st["g"], 0.0, a["gscale"], coef)
    mi = s(b1).fma(exact(st["m"]), s(BT._om(b1)).mul(gi, 1))
    vi = s(b2).fma(exact(st["v"]), s(BT._om(b2)).mul(gi, 1).mul(gi, 1))
    vi = Interval(vi.lo.clamp_min(0.0), vi.hi)
    den = vi.sqrt().div(s(bc2s), 1).add(s(eps), 1)
    u = mi.div(s(bc1), 1).div(den, 1)
    if f32(wd) != 0.0:
        u = s(f32(wd)).mul(exact(st["p"]), 1).add(u, 1)
    return u, mi, vi


def lamb_intervals(st, a, lr, wd, r, coef=None):
    """p = fl(p - fl(fl(lr r) u)) with r the ratio the device stored (exact data)"""
    u, mi, vi = lamb_direction(st, a, wd, coef)
    s = lambda c: exact(c, like=st["g"])
    step = s(f32(lr)).mul(s(float(r)), 1)
    return dict(p=exact(st["p"]).add(step.mul(u, 1), 1, -1.0), m=mi, v=vi)


def lars_intervals(st, a, lr, wd, r, coef=None):
    """gi = fl(fmaf(wd, p, gs) r), then bounds_tail's SGD update"""
    gi = BT._opt_grad(st["p"], st["g"], wd, a["gscale"], coef).mul(exact(float(r), like=st["g"]), 1)
    return _update("sgd", exact(st["p"]), gi, st, a, lr)


def root_hull(iv):
    """(lo, hi) of sqrt(sum x^2) over every x inside iv, as floats (the derivation in the module docstring)"""
    lo_abs = torch.where((iv.lo <= 0) & (iv.hi >= 0), torch.zeros_like(iv.lo), torch.minimum(iv.lo.abs(), iv.hi.abs()))
    hi_abs = torch.maximum(iv.lo.abs(), iv.hi.abs())
    return float(torch.sqrt((lo_abs * lo_abs).sum())), float(torch.sqrt((hi_abs * hi_abs).sum()))


def lamb_ratio_hull(w_ref, u_iv):
    """-> (un_lo, un_hi, r_lo, r_hi): un's hull widened by 2^-24, r's by 2^-22; w_ref: the exact fp64 weight norm (> 0), un_lo > 0"""
    lo, hi = root_hull(u_iv)
    return lo * (1 - 2.0 ** -24), hi * (1 + 2.0 ** -24), w_ref / hi * (1 - 2.0 ** -22), w_ref / lo * (1 + 2.0 ** -22)


LARS_RATIO_REL = 2.0 ** -21         # lars_ratio_bound: see the module docstring


def slice_state(st, a, b):
    return {k: v[a:b] for k, v in st.items()}


# ---- the trust-ratio tests' data (pure host data: the CPU suite checks the hulls are narrow, the GPU suite uses them) ---------------------
GROUPS3 = [(1e-3, 1e-2), (3e-3, 0.0), (5e-4, 5e-2)]                   # (lr, weight_decay) of the three groups
ADAM = dict(b1=0.9, b2=0.999, eps=1e-8, step=2, gscale=0.125)
RMSPROP = dict(alpha=0.99, eps=1e-8, momentum=0.9, gscale=1.0 / 3)
SGD = dict(momentum=0.9, dampening=0.5, nesterov=0, step=2, gscale=0.125)
ZERO_P_SEG, ZERO_G_SEG = 3, 4      # segment 3 (255 elements, group 0): p == 0; segment 4 (257 elements, group 1, wd 0): g == m == 0


def flat_state(layout, seed):
    """bounds_tail.opt_data over the whole flat buffer, plus an EMA shadow"""
    n = layout[0][-1][1]
    p, g, m, v, buf = BT.opt_data(n, seed=seed)
    return dict(p=p, g=g, m=m, v=v, buf=buf, ema=p * 0.75 + 0.01)


def trust_state(layout, tb, seed=5):
    """flat_state with the rules' corner cases: an all-zero weight tensor and a tensor without gradient or first moment"""
    st = flat_state(layout, seed)
    a, n = tb.segs[ZERO_P_SEG][:2]
    st["p"][a:a + n] = 0.0
    a, n = tb.segs[ZERO_G_SEG][:2]
    st["g"][a:a + n] = 0.0
    st["m"][a:a + n] = 0.0
    return st
