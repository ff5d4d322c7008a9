"""The access model of the launch lists: for every opcode of _lib.OP_SLOTS and every pointer slot of it, which bytes a launch
reads, writes or reads-and-writes, as a function of the op's own integers and doubles (and, for descriptor arrays, of the
descriptors).  tests/plan_verify.py checks the planner's lists against it on the CPU; tests/test_gpu_plan_access.py holds it to what
the kernels touch.

Conventions
  - ACCESS[opcode][slot] is a function (f, lib, ptr, peek) -> [(mode, first byte, number of bytes), ...].  f: the op's integers and
    doubles by slot name; lib: the loaded library (the host-side queries the planner itself asks); ptr: the slot's pointer, never
    null (a null slot carries no access and is not asked); peek(ptr, nbytes): the bytes of a descriptor array.
  - mode R: only read.  W: every byte of the range is written and its old value does not reach any result.  RW: the old value
    reaches the new one (accumulate=1 targets, the running statistics, the in-place folds of a weight-gradient table).
  - A table that is touched in rows is a list of ranges, one per row; the same byte may be in an R and in a W range of one slot (the
    fold rows of a two-level reduction: read as partial sums, then overwritten with the chunk's sum).
  - An empty list: the slot is set but this launch does not touch it (the planner hands one geometry to both launches of a split
    depthwise backward; the level-2 task of mnas_bwd_post carries the gradient pointer its level 3 will use).
  - Layouts are those of include/mnas.h.  Loads that a mask discards are not modelled: a range says which bytes can reach a result.

EXEMPT lists the (opcode, slot) pairs without a model.  It is empty."""
import ctypes

from mnasnet_pytorch_amd import _lib as L

R, W, RW = "r", "w", "rw"
BF16, F32 = 2, 4
FIN_SPLITS = 128            # csrc/mnas_elementwise.hip: rows per chunk of a two-level weight-gradient reduction

EXEMPT = ()


def _none(f, lib, ptr, peek):
    return []


def _act(prefix, rows, C):
    """act-on-load triple: bf16 [rows][C] and the two coefficient rows (bnbuf rows 0 and 1, addressed by their own pointers)"""
    return {prefix + ".data": lambda f, lib, p, peek: [(R, p, rows(f) * C(f) * BF16)],
            prefix + ".scale": lambda f, lib, p, peek: [(R, p, C(f) * F32)],
            prefix + ".shift": lambda f, lib, p, peek: [(R, p, C(f) * F32)]}


def _grad(prefix, rows, C):
    """dy-on-load triple: g and y bf16 [rows][C], coef = bnbuf rows 0..4"""
    return {prefix + ".g": lambda f, lib, p, peek: [(R, p, rows(f) * C(f) * BF16)],
            prefix + ".y": lambda f, lib, p, peek: [(R, p, rows(f) * C(f) * BF16)],
            prefix + ".coef": lambda f, lib, p, peek: [(R, p, 5 * C(f) * F32)]}


def _red_bn(C):
    """the fused BatchNorm-backward reduce reads rows 0, 1 (the ReLU mask) and 5, 6 (xhat) of the producer's block"""
    return lambda f, lib, p, peek: [(R, p, 2 * C(f) * F32), (R, p + 5 * C(f) * F32, 2 * C(f) * F32)]


def _table(mode, C, cols):
    """float[2][C][cols]: statistics and reduce partials"""
    return lambda f, lib, p, peek: [(mode, p, 2 * C(f) * cols(f, lib) * F32)]


def _plain(mode, nbytes):
    return lambda f, lib, p, peek: [(mode, p, nbytes(f))]


def _acc(flag, nbytes):
    """a gradient target: accumulated into (accumulate != 0) or overwritten"""
    return lambda f, lib, p, peek: [(RW if f[flag] else W, p, nbytes(f))]


def _fin_partial(nsplit, total):
    """the table of mnas_wgrad_finalize / mnas_dw_wgrad_finalize: every row is read; with more than 2 * FIN_SPLITS rows the first
    row of every FIN_SPLITS-row chunk then receives the chunk's sum"""
    def fn(f, lib, p, peek):
        n, t = nsplit(f), total(f) * F32
        out = [(R, p, n * t)]
        if n > 2 * FIN_SPLITS:
            out += [(W, p + c * FIN_SPLITS * t, t) for c in range(-(-n // FIN_SPLITS))]
        return out
    return fn


def _post_total(f, w):
    return f[w + ".Co"] * f[w + ".taps"] * (1 if f[w + ".dw"] else f[w + ".Ci"])


def _post_partial(w):
    """MnasPostWgrad.partial by level: 1 = all rows read; 2 = all rows read, chunk heads overwritten; 3 = the chunk heads read"""
    def fn(f, lib, p, peek):
        lvl, n, t = f[w + ".level"], f[w + ".nsplit"], _post_total(f, w) * F32
        heads = [p + c * FIN_SPLITS * t for c in range(-(-n // FIN_SPLITS))]
        if lvl == 1:
            return [(R, p, n * t)]
        if lvl == 2:
            return [(R, p, n * t)] + [(W, h, t) for h in heads]
        if lvl == 3:
            return [(R, h, t) for h in heads]
        return []
    return fn


def _post_grad(w):
    return lambda f, lib, p, peek: [(RW, p, _post_total(f, w) * F32)] if f[w + ".level"] in (1, 3) else []


def _post_slots(frozen):
    bn = lambda f: f["bn_C"] > 0
    C = lambda f: f["bn_C"]
    d = {"bn_partial": lambda f, lib, p, peek: [(R, p, 2 * C(f) * f["bn_nparts"] * F32)] if bn(f) else [],
         # rows 0 (s), 5 (mean), 6 (invstd) are read; rows 2..4 (c1..c3) written unless the statistics are frozen
         "bnbuf": lambda f, lib, p, peek: ([(R, p, C(f) * F32), (R, p + 5 * C(f) * F32, 2 * C(f) * F32)]
                                          + ([] if frozen else [(W, p + 2 * C(f) * F32, 3 * C(f) * F32)])) if bn(f) else [],
         "dgamma": lambda f, lib, p, peek: [(RW, p, C(f) * F32)] if bn(f) else [],
         "dbeta": lambda f, lib, p, peek: [(RW, p, C(f) * F32)] if bn(f) else [],
         "w1.partial": _post_partial("w1"), "w1.grad": _post_grad("w1"),
         "w2.partial": _post_partial("w2"), "w2.grad": _post_grad("w2")}
    if frozen:
        d["dbias"] = lambda f, lib, p, peek: [(RW, p, C(f) * F32)] if bn(f) else []
    return d


def _bn_bwd_fin(frozen):
    C = lambda f: f["C"]
    d = {"partial": _table(R, C, lambda f, lib: f["nparts"]),
         "bnbuf": lambda f, lib, p, peek: [(R, p, C(f) * F32), (R, p + 5 * C(f) * F32, 2 * C(f) * F32)]
         + ([] if frozen else [(W, p + 2 * C(f) * F32, 3 * C(f) * F32)]),
         "dgamma": _acc("accumulate", lambda f: C(f) * F32), "dbeta": _acc("accumulate", lambda f: C(f) * F32)}
    if frozen:
        d["dbias"] = _acc("accumulate", lambda f: C(f) * F32)
    return d


def _isqrt_taps(taps):
    k = int(round(taps ** 0.5))
    if k * k != taps:
        raise ValueError("taps %d is no square" % taps)
    return k


def _pack_ranges(lib, kind, Co, Ci, kh, kw, w, dst):
    src = Co * kh * kw * F32 if kind == L.PACK_DW else Co * Ci * kh * kw * F32
    return [(R, w, src), (W, dst, lib.mnas_packed_bytes(kind, Co, Ci, kh, kw))]


def _pack_batch(f, lib, p, peek):
    """the descriptor array is read, and through it every source weight (read) and packed destination (written)"""
    n, size = f["n"], ctypes.sizeof(L.MnasPackDesc)
    out = [(R, p, n * size)]
    for d in (L.MnasPackDesc * n).from_buffer_copy(peek(p, n * size)):
        k = _isqrt_taps(d.taps)
        out += _pack_ranges(lib, d.kind, d.Co, 1 if d.kind == L.PACK_DW else d.Ci, k, k, d.w, d.dst)
    return out


def _frozen_batch(f, lib, p, peek):
    """the descriptor array, the four per-channel inputs of every application, rows 0..6 of its block"""
    n, size = f["n"], ctypes.sizeof(L.MnasBnFrozenDesc)
    out = [(R, p, n * size)]
    for d in (L.MnasBnFrozenDesc * n).from_buffer_copy(peek(p, n * size)):
        out += [(R, q, d.C * F32) for q in (d.gamma, d.beta, d.running_mean, d.running_var)]
        out.append((W, d.bnbuf, 7 * d.C * F32))
    return out


def _dw_ho(f):
    if f["stride"] == 2:
        return ((f["H"] + 2 * (f["k"] // 2) - f["k"]) // 2 + 1, (f["W"] + 2 * (f["k"] // 2) - f["k"]) // 2 + 1)
    return f["H"], f["W"]


def _dw_rows(f, lib, which):
    r = lib.mnas_dw_rows(f["N"], f["H"], f["W"], f["C"], f["k"], f["nparts"], which)
    if r < 1:
        raise ValueError("mnas_dw_rows refuses %s which=%d" % (dict(f), which))
    return r


def _dw_bwd():
    C = lambda f: f["C"]
    px_in = lambda f: f["N"] * f["H"] * f["W"]
    px_out = lambda f: f["N"] * _dw_ho(f)[0] * _dw_ho(f)[1]
    s2 = lambda f: f["stride"] == 2

    def wpartial(f, lib, p, peek):
        if f["phase"] == 1:
            return []
        rows = _dw_rows(f, lib, 7 if s2(f) else (1 if f["phase"] == 0 else 3))
        return [(W, p, rows * f["k"] * f["k"] * C(f) * F32)]

    def red_partial(f, lib, p, peek):
        if f["phase"] == 2 or s2(f):
            return []
        return [(W, p, 2 * C(f) * _dw_rows(f, lib, 1 if f["phase"] == 0 else 2) * F32)]

    red_bn = _red_bn(C)
    d = dict(_act("x", px_in, C))
    d.update(_grad("dy", px_out, C))
    d.update({"w": _plain(R, lambda f: f["k"] * f["k"] * C(f) * F32),
              "gin": lambda f, lib, p, peek: [] if f["phase"] == 2 else [(W, p, px_in(f) * C(f) * BF16)],
              "wpartial": wpartial,
              "red_bn": lambda f, lib, p, peek: [] if (f["phase"] == 2 or s2(f)) else red_bn(f, lib, p, peek),
              "red_partial": red_partial})
    return d


def _conv_gemm():
    px_in = lambda f: f["N"] * f["Hi"] * f["Wi"]
    px_out = lambda f: f["N"] * f["Ho"] * f["Wo"]
    Ci, Co = (lambda f: f["Ci"]), (lambda f: f["Co"])
    d = dict(_act("act", px_in, Ci))
    d.update(_grad("grad", px_in, Ci))
    d.update({
        # mode 1 names the conv by its gradient: the op's (Ci, Co) are the forward's (Co, Ci)
        "w": lambda f, lib, p, peek: [(R, p, lib.mnas_packed_bytes(L.PACK_FWD, f["Co"], f["Ci"], f["kh"], f["kw"]) if f["mode"] == 0
                                       else lib.mnas_packed_bytes(L.PACK_DGRAD, f["Ci"], f["Co"], f["kh"], f["kw"]))],
        "bias": _plain(R, lambda f: Co(f) * F32),
        "resid": _plain(R, lambda f: px_out(f) * Co(f) * BF16),
        "out": _plain(W, lambda f: px_out(f) * Co(f) * BF16),
        "stats": _table(W, Co, lambda f, lib: f["nparts"]),
        "red_y": _plain(R, lambda f: px_out(f) * Co(f) * BF16),
        "red_bn": _red_bn(Co),
        "gate": _plain(R, lambda f: f["N"] * Ci(f) * F32)})
    return d


def _conv_wgrad():
    Ci, Co = (lambda f: f["Ci"]), (lambda f: f["Co"])
    d = dict(_act("x", lambda f: f["N"] * f["Hi"] * f["Wi"], Ci))
    d.update(_grad("dy", lambda f: f["N"] * f["Ho"] * f["Wo"], Co))
    d["partial"] = _plain(W, lambda f: f["nsplit"] * Co(f) * f["kh"] * f["kw"] * Ci(f) * F32)
    return d


def _pw_bwd():
    M, Ci, Co = (lambda f: f["M"]), (lambda f: f["Ci"]), (lambda f: f["Co"])
    d = dict(_act("x", M, Ci))
    d.update(_grad("dy", M, Co))
    d.update({"w": lambda f, lib, p, peek: [(R, p, lib.mnas_packed_bytes(L.PACK_DGRAD, Co(f), Ci(f), 1, 1))],
              "resid": _plain(R, lambda f: M(f) * Ci(f) * BF16),
              "gin": _plain(W, lambda f: M(f) * Ci(f) * BF16),
              "wpartial": _plain(W, lambda f: f["nparts"] * Co(f) * Ci(f) * F32),
              "red_partial": _table(W, Ci, lambda f, lib: f["nparts"]),
              "red_y": _plain(R, lambda f: M(f) * Ci(f) * BF16),
              "red_bn": _red_bn(Ci),
              "w_fwd": lambda f, lib, p, peek: [(R, p, lib.mnas_packed_bytes(L.PACK_FWD, Co(f), Ci(f), 1, 1))],
              "b_fwd": _plain(R, lambda f: Co(f) * F32)})
    return d


def _stem(kind):
    img = lambda f: f["N"] * 3 * f["H"] * f["W"]
    px = lambda f: f["N"] * f["Ho"] * f["Wo"]
    Co = lambda f: f["Co"]
    x = _plain(R, lambda f: img(f) * (1 if f["in_u8"] else F32))
    aff = _plain(R, lambda f: 6 * F32)
    if kind == "fwd":
        return {"x": x, "w": lambda f, lib, p, peek: [(R, p, lib.mnas_packed_bytes(L.PACK_FWD, Co(f), 27, 1, 1))],
                "bias": _plain(R, lambda f: Co(f) * F32), "out": _plain(W, lambda f: px(f) * Co(f) * BF16),
                "stats": _table(W, Co, lambda f, lib: f["nparts"]), "in_affine": aff}
    if kind == "wgrad":
        d = {"x": x, "partial": _plain(W, lambda f: f["nparts"] * Co(f) * 27 * F32), "in_affine": aff}
        d.update(_grad("dy", px, Co))
        return d
    d = {"w": _plain(R, lambda f: Co(f) * 27 * F32), "in_affine": aff, "dx": _plain(W, lambda f: img(f) * F32)}
    d.update(_grad("dy", px, Co))
    return d


def _bn_fwd_fin():
    C = lambda f: f["C"]
    tr = lambda f: bool(f["training"])
    row = lambda f: C(f) * F32
    return {"partial": lambda f, lib, p, peek: [(R, p, 2 * C(f) * f["nparts"] * F32)] if tr(f) else [],
            "gamma": _plain(R, row), "beta": _plain(R, row),
            "rmean": lambda f, lib, p, peek: [(RW if tr(f) else R, p, row(f))],
            "rvar": lambda f, lib, p, peek: [(RW if tr(f) else R, p, row(f))],
            "nbt": lambda f, lib, p, peek: [(RW, p, 8)] if tr(f) else [],
            # rows 0, 1 always; rows 5, 6 (batch mean, invstd) from batch statistics only
            "bnbuf": lambda f, lib, p, peek: [(W, p, 2 * row(f))] + ([(W, p + 5 * row(f), 2 * row(f))] if tr(f) else [])}


def _head_linear():
    NI, NO, OI = (lambda f: f["N"] * f["I"] * F32), (lambda f: f["N"] * f["O"] * F32), (lambda f: f["O"] * f["I"] * F32)

    def when(which, mode, nbytes):
        return lambda f, lib, p, peek: [((RW if f["accumulate"] else W) if mode == "acc" else mode, p, nbytes(f))] \
            if f["which"] in which else []
    return {"x": when((0, 1), R, NI), "w": when((0, 2), R, OI), "b": when((0,), R, lambda f: f["O"] * F32), "y": when((0,), W, NO),
            "dz": when((1, 2), R, NO), "dw": when((1,), "acc", OI), "db": when((1,), "acc", lambda f: f["O"] * F32),
            "dx": when((2,), W, NI), "relu_mask": when((2,), R, NI)}


def _se_proj_fin():
    slab = lambda f: f["Co"] * f["Ci"] * F32
    NC = lambda f: f["N"] * f["Ci"] * F32
    return {
        # every slab is read; the first slab of every image then holds the image's gated sum (read again by the second kernel)
        "wpartial": lambda f, lib, p, peek: [(R, p, f["N"] * f["kseg"] * slab(f))]
        + [(W, p + n * f["kseg"] * slab(f), slab(f)) for n in range(f["N"])],
        "u": _plain(R, NC), "w": _plain(R, slab), "grad": _acc("accumulate", slab), "du": _plain(W, NC)}


def _se_scratch(f, lib, p, peek):
    b = lib.mnas_se_scratch_bytes(f["N"], f["HW"], f["C"])
    if b < 0:
        raise ValueError("mnas_se_scratch_bytes refuses %s" % (dict(f),))
    return [(W, p, b)]


def _se_cols(f, lib):
    c = lib.mnas_se_bwd_apply_cols(f["N"], f["HW"], f["C"])
    if c < 1:
        raise ValueError("mnas_se_bwd_apply_cols refuses %s" % (dict(f),))
    return c


def _merge(*dicts):
    out = {}
    for d in dicts:
        out.update(d)
    return out


_rowsd = lambda f: int(f["rows"])
_C = lambda f: f["C"]
_NHWC = lambda f: f["N"] * f["HW"] * f["C"] * BF16
_NC = lambda f: f["N"] * f["C"] * F32
_NE, _NR, _RE = (lambda f: f["N"] * f["E"] * F32), (lambda f: f["N"] * f["R"] * F32), (lambda f: f["R"] * f["E"] * F32)

ACCESS = {
    L.OP_CONV_GEMM: _conv_gemm(),
    L.OP_CONV_WGRAD: _conv_wgrad(),
    L.OP_WGRAD_FINALIZE: {"partial": _fin_partial(lambda f: f["nsplit"], lambda f: f["Co"] * f["Ci"] * f["taps"]),
                          "grad": _acc("accumulate", lambda f: f["Co"] * f["Ci"] * f["taps"] * F32)},
    L.OP_DW_FWD: _merge(_act("in_", lambda f: f["N"] * f["H"] * f["W"], _C), {
        "w": _plain(R, lambda f: f["k"] * f["k"] * f["C"] * F32), "bias": _plain(R, lambda f: f["C"] * F32),
        "out": _plain(W, lambda f: f["N"] * _dw_ho(f)[0] * _dw_ho(f)[1] * f["C"] * BF16),
        "stats": _table(W, _C, lambda f, lib: _dw_rows(f, lib, 4 if f["stride"] == 2 else 0))}),
    L.OP_DW_BWD: _dw_bwd(),
    L.OP_DW_WGRAD_FINALIZE: {"wpartial": _fin_partial(lambda f: f["nparts"], lambda f: f["C"] * f["k"] * f["k"]),
                             "grad": _acc("accumulate", lambda f: f["C"] * f["k"] * f["k"] * F32)},
    L.OP_STEM_FWD: _stem("fwd"),
    L.OP_STEM_WGRAD: _stem("wgrad"),
    L.OP_STEM_DGRAD: _stem("dgrad"),
    L.OP_BN_FWD_FINALIZE: _bn_fwd_fin(),
    L.OP_BN_BWD_REDUCE: {"g": _plain(R, lambda f: _rowsd(f) * f["C"] * BF16), "y": _plain(R, lambda f: _rowsd(f) * f["C"] * BF16),
                         "bnbuf": _red_bn(_C), "partial": _table(W, _C, lambda f, lib: f["nparts"])},
    L.OP_BN_BWD_FINALIZE: _bn_bwd_fin(False),
    L.OP_BN_BWD_FINALIZE_FROZEN: _bn_bwd_fin(True),
    L.OP_ADD_ACT: _merge(_act("a", _rowsd, _C), _act("b", _rowsd, _C), {
        "out_bf16": _plain(W, lambda f: _rowsd(f) * f["C"] * BF16), "out_nchw": _plain(W, lambda f: _rowsd(f) * f["C"] * F32)}),
    L.OP_NCHW_TO_NHWC: {"src": _plain(R, lambda f: f["N"] * f["C"] * f["HW"] * F32), "dst": _plain(W, _NHWC)},
    L.OP_PACK_WEIGHTS: {
        "w": lambda f, lib, p, peek: [_pack_ranges(lib, f["kind"], f["Co"], f["Ci"], f["kh"], f["kw"], p, 0)[0]],
        "dst": lambda f, lib, p, peek: [_pack_ranges(lib, f["kind"], f["Co"], f["Ci"], f["kh"], f["kw"], 0, p)[1]]},
    L.OP_PACK_BATCH: {"descs": _pack_batch},
    L.OP_EVENT_RECORD: {"event": _none, "gate": _none},        # handles and a host int: no device memory
    L.OP_EVENT_WAIT: {"event": _none},
    L.OP_PW_BWD: _pw_bwd(),
    L.OP_POOL_ACT: _merge(_act("a", lambda f: f["N"] * f["HW"], _C), {"out": _plain(W, _NC)}),
    L.OP_POOL_BWD: {"gpool": _plain(R, _NC), "g": _plain(W, _NHWC)},
    L.OP_DY_MAT: _merge(_grad("dy", _rowsd, _C), {"out": _plain(W, lambda f: _rowsd(f) * f["C"] * BF16)}),
    L.OP_BWD_POST: _post_slots(False),
    L.OP_BWD_POST_FROZEN: _post_slots(True),
    L.OP_BN_FROZEN_BATCH: {"descs": _frozen_batch},
    L.OP_TCONV_DGRAD: {
        "dy": _plain(R, lambda f: f["N"] * f["Ho"] * f["Wo"] * f["Co"] * BF16),
        "w": lambda f, lib, p, peek: [(R, p, lib.mnas_packed_bytes(L.PACK_TCONV, f["Co"], f["Ci"], 3, 3))],
        "out": _plain(W, lambda f: f["N"] * 4 * f["Ho"] * f["Wo"] * f["Ci"] * BF16),
        "stats": _table(W, lambda f: f["Ci"], lambda f, lib: f["nparts"]),
        "red_y": _plain(R, lambda f: f["N"] * 4 * f["Ho"] * f["Wo"] * f["Ci"] * BF16),
        "red_bn": _red_bn(lambda f: f["Ci"])},
    L.OP_HEAD_LINEAR: _head_linear(),
    L.OP_SE_SCALE: _merge(_act("a", lambda f: f["N"] * f["HW"], _C), {"u": _plain(R, _NC), "out": _plain(W, _NHWC)}),
    L.OP_SE_BWD_REDUCE: _merge(_act("a", lambda f: f["N"] * f["HW"], _C), {
        "gs": _plain(R, _NHWC), "u": _plain(R, _NC), "du": _plain(W, _NC), "scratch": _se_scratch}),
    L.OP_SE_BWD_APPLY: {"gs": _plain(R, _NHWC), "u": _plain(R, _NC), "dz": _plain(R, _NC), "out": _plain(W, _NHWC),
                        "red_y": _plain(R, _NHWC), "red_bn": _red_bn(_C), "red_partial": _table(W, _C, _se_cols)},
    L.OP_SE_GATE: {"u": _plain(R, _NC), "gate": _plain(W, _NC)},
    L.OP_SE_PROJ_FIN: _se_proj_fin(),
    L.OP_SE_FC_FWD: {"z": _plain(R, _NE), "w1": _plain(R, _RE), "b1": _plain(R, lambda f: f["R"] * F32), "w2": _plain(R, _RE),
                     "b2": _plain(R, lambda f: f["E"] * F32), "hb": _plain(W, _NR), "u": _plain(W, _NE), "gate": _plain(W, _NE)},
    L.OP_SE_FC_BWD: {"du": _plain(R, _NE), "z": _plain(R, _NE), "hb": _plain(R, _NR), "w1": _plain(R, _RE), "w2": _plain(R, _RE),
                     "dh": _plain(W, _NR), "dz": _plain(W, _NE), "dw1": _acc("accumulate", _RE),
                     "db1": _acc("accumulate", lambda f: f["R"] * F32), "dw2": _acc("accumulate", _RE),
                     "db2": _acc("accumulate", lambda f: f["E"] * F32)},
}


def model_keys(access=None):
    """{(opcode, pointer slot)} the model covers"""
    access = ACCESS if access is None else access
    return {(opc, name) for opc, slots in access.items() for name in slots}


def slot_keys(op_slots=None):
    """{(opcode, pointer slot)} of _lib.OP_SLOTS, retired (None) slots left out"""
    op_slots = L.OP_SLOTS if op_slots is None else op_slots
    return {(opc, name) for opc, kinds in op_slots.items() for name in kinds[2] if name is not None}


def check_model_covers_slots(access=None, op_slots=None):
    """The model's key set is OP_SLOTS' pointer slots, exactly, apart from EXEMPT.  Returns (unmodelled, unknown)."""
    have, want = model_keys(access) | set(EXEMPT), slot_keys(op_slots)
    return sorted(want - have), sorted(have - want)


def op_fields(o):
    """the op's named integers and doubles"""
    ints, dbls, _ = L.OP_SLOTS[o.opcode]
    f = {name: int(o.i[k]) for k, name in enumerate(ints) if name is not None}
    f.update({name: float(o.d[k]) for k, name in enumerate(dbls) if name is not None})
    return f


def op_accesses(o, lib, peek):
    """[(slot name, mode, first byte, bytes)] of one op: every non-null pointer slot through its model; empty ranges dropped"""
    f, out = op_fields(o), []
    for k, name in enumerate(L.OP_SLOTS[o.opcode][2]):
        if name is None or not o.p[k]:
            continue
        for mode, start, n in ACCESS[o.opcode][name](f, lib, int(o.p[k]), peek):
            if n > 0:
                out.append((name, mode, start, n))
    return out
