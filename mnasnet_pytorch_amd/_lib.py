"""ctypes binding of libmnas_hip.so (include/mnas.h).  No CPU fallback: if the library is missing the
import of the product path fails loudly; if a launcher returns non-zero a RuntimeError is raised."""
from __future__ import annotations

import ctypes as C
import os

import torch  # imported first so that libamdhip64.so.7 resolves to the copy torch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 8          # include/mnas.h: mnas_version()
LIB_PATH = os.environ.get("MNAS_LIB_PATH") or os.path.join(_HERE, "csrc", "libmnas_hip.so")      # override: A/B builds (tools/)

c_void_p, c_int, c_float, c_double, c_int64 = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_int64


class MnasActIn(C.Structure):
    _fields_ = [("data", c_void_p), ("scale", c_void_p), ("shift", c_void_p)]


class MnasGradIn(C.Structure):
    _fields_ = [("g", c_void_p), ("y", c_void_p), ("coef", c_void_p)]


class MnasConvGemm(C.Structure):
    _fields_ = [("mode", C.c_int32), ("N", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Ci", C.c_int32),
                ("Ho", C.c_int32), ("Wo", C.c_int32), ("Co", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("stride", C.c_int32), ("pad", C.c_int32), ("nparts", C.c_int32), ("reserved", C.c_int32),
                ("act", MnasActIn), ("grad", MnasGradIn), ("w", c_void_p), ("bias", c_void_p), ("resid", c_void_p),
                ("out", c_void_p), ("stats", c_void_p), ("red_y", c_void_p), ("red_bn", c_void_p), ("gate", c_void_p)]


class MnasConvWgrad(C.Structure):
    _fields_ = [("N", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Ci", C.c_int32), ("Ho", C.c_int32),
                ("Wo", C.c_int32), ("Co", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32),
                ("pad", C.c_int32), ("nsplit", C.c_int32), ("x", MnasActIn), ("dy", MnasGradIn), ("partial", c_void_p)]


class MnasDwFwd(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("k", C.c_int32),
                ("nparts", C.c_int32), ("in_", MnasActIn), ("w", c_void_p), ("bias", c_void_p), ("out", c_void_p),
                ("stats", c_void_p), ("stride", C.c_int32), ("reserved", C.c_int32)]


class MnasDwBwd(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("k", C.c_int32),
                ("nparts", C.c_int32), ("x", MnasActIn), ("dy", MnasGradIn), ("w", c_void_p), ("gin", c_void_p),
                ("wpartial", c_void_p), ("red_bn", c_void_p), ("red_partial", c_void_p), ("phase", C.c_int32),
                ("stride", C.c_int32), ("g_masked", C.c_int32), ("reserved", C.c_int32)]


class MnasPwBwd(C.Structure):
    _fields_ = [("M", C.c_int32), ("Ci", C.c_int32), ("Co", C.c_int32), ("nparts", C.c_int32), ("x", MnasActIn),
                ("dy", MnasGradIn), ("w", c_void_p), ("resid", c_void_p), ("gin", c_void_p), ("wpartial", c_void_p),
                ("red_partial", c_void_p), ("red_y", c_void_p), ("red_bn", c_void_p), ("w_fwd", c_void_p),
                ("b_fwd", c_void_p), ("gin_masked", C.c_int32), ("seg_px", C.c_int32)]


class MnasPostWgrad(C.Structure):
    _fields_ = [("partial", c_void_p), ("grad", c_void_p), ("nsplit", C.c_int32), ("Co", C.c_int32), ("Ci", C.c_int32),
                ("taps", C.c_int32), ("dw", C.c_int32), ("level", C.c_int32)]


class MnasBwdPost(C.Structure):
    _fields_ = [("bn_partial", c_void_p), ("bnbuf", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p), ("count", c_double),
                ("bn_nparts", C.c_int32), ("bn_C", C.c_int32), ("w1", MnasPostWgrad), ("w2", MnasPostWgrad)]


class MnasBwdPostFrozen(C.Structure):
    _fields_ = MnasBwdPost._fields_ + [("dbias", c_void_p)]


class MnasBnFrozenDesc(C.Structure):
    _fields_ = [("gamma", c_void_p), ("beta", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p), ("bnbuf", c_void_p),
                ("C", C.c_int32), ("eps", c_float)]


class MnasTconvDgrad(C.Structure):
    _fields_ = [("N", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("Co", C.c_int32), ("Ci", C.c_int32),
                ("nparts", C.c_int32), ("dy", c_void_p), ("w", c_void_p), ("out", c_void_p), ("stats", c_void_p),
                ("red_y", c_void_p), ("red_bn", c_void_p)]


class MnasPackDesc(C.Structure):
    _fields_ = [("w", c_void_p), ("dst", c_void_p), ("kind", C.c_int32), ("Co", C.c_int32), ("Ci", C.c_int32),
                ("taps", C.c_int32)]


class MnasStemFwd(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
                ("Co", C.c_int32), ("nparts", C.c_int32), ("x", c_void_p), ("w", c_void_p), ("bias", c_void_p),
                ("out", c_void_p), ("stats", c_void_p), ("in_affine", c_void_p), ("in_u8", C.c_int32), ("reserved", C.c_int32)]


class MnasStemWgrad(C.Structure):
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
                ("Co", C.c_int32), ("nparts", C.c_int32), ("x", c_void_p), ("dy", MnasGradIn), ("partial", c_void_p),
                ("in_affine", c_void_p), ("in_u8", C.c_int32), ("reserved", C.c_int32)]


class MnasImgXform(C.Structure):
    _fields_ = [("src_offset", c_int64), ("src_h", C.c_int32), ("src_w", C.c_int32), ("src_c", C.c_int32),
                ("src_stride", C.c_int32), ("box_top", C.c_int32), ("box_left", C.c_int32), ("box_h", C.c_int32),
                ("box_w", C.c_int32), ("rh", C.c_int32), ("rw", C.c_int32), ("win_top", C.c_int32), ("win_left", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


IMGX_HFLIP, IMGX_VFLIP = 1, 2         # MNAS_IMGX_HFLIP / _VFLIP


class MnasImgColor(C.Structure):
    _fields_ = [("nops", C.c_int32), ("op", C.c_int32 * 5), ("factor", C.c_float * 5), ("hue_shift", C.c_int32),
                ("reserved", C.c_int32)]


IMGC_BRIGHTNESS, IMGC_CONTRAST, IMGC_SATURATION, IMGC_HUE, IMGC_GRAY = 1, 2, 3, 4, 5     # MNAS_IMGC_*
IMGC_MAX_OPS = 5
IMGC_NCHW, IMGC_NHWC = 0, 1


class MnasImgMix(C.Structure):
    _fields_ = [("mode", C.c_int32), ("partner", C.c_int32), ("w16", C.c_int32), ("y0", C.c_int32), ("x0", C.c_int32),
                ("y1", C.c_int32), ("x1", C.c_int32), ("reserved", C.c_int32)]


IMGM_NONE, IMGM_MIXUP, IMGM_CUTMIX = 0, 1, 2         # MNAS_IMGM_*


class MnasImgAug(C.Structure):
    _fields_ = [("nops", C.c_int32), ("op", C.c_int32 * 4), ("factor", C.c_float * 4), ("arg", (C.c_int32 * 6) * 4),
                ("reserved", C.c_int32)]


(IMGA_IDENTITY, IMGA_AFFINE, IMGA_BRIGHTNESS, IMGA_COLOR, IMGA_CONTRAST, IMGA_SHARPNESS, IMGA_POSTERIZE, IMGA_SOLARIZE, IMGA_INVERT,
 IMGA_AUTOCONTRAST, IMGA_EQUALIZE) = range(11)         # MNAS_IMGA_*
IMGA_MAX_OPS = 4


class MnasImgErase(C.Structure):
    _fields_ = [("mode", C.c_int32), ("y0", C.c_int32), ("x0", C.c_int32), ("y1", C.c_int32), ("x1", C.c_int32),
                ("fill", C.c_uint8 * 3), ("pad", C.c_uint8), ("reserved", C.c_int32 * 2)]


IMGE_NONE, IMGE_CONST, IMGE_NOISE = 0, 1, 2          # MNAS_IMGE_*
IMGE_TABLE = 4096                                     # table entries per channel


class MnasOp(C.Structure):
    _fields_ = [("opcode", C.c_int32), ("i", C.c_int32 * 15), ("d", C.c_double * 4), ("p", c_void_p * 16)]


OP_CONV_GEMM, OP_CONV_WGRAD, OP_WGRAD_FINALIZE, OP_DW_FWD, OP_DW_BWD, OP_DW_WGRAD_FINALIZE = 1, 2, 3, 4, 5, 6
OP_STEM_FWD, OP_STEM_WGRAD, OP_BN_FWD_FINALIZE, OP_BN_BWD_REDUCE, OP_BN_BWD_FINALIZE = 7, 8, 9, 10, 11
OP_ADD_ACT, OP_NCHW_TO_NHWC, OP_PACK_WEIGHTS, OP_EVENT_RECORD, OP_EVENT_WAIT, OP_PW_BWD, OP_PACK_BATCH = 12, 13, 14, 15, 16, 17, 18
OP_POOL_ACT, OP_POOL_BWD, OP_DY_MAT = 22, 23, 24          # 19-21, 27-29, 36: retired in ABI 6 (include/mnas.h)
OP_BWD_POST, OP_TCONV_DGRAD = 25, 26
OP_HEAD_LINEAR, OP_SE_SCALE, OP_SE_BWD_REDUCE, OP_SE_BWD_APPLY = 30, 31, 32, 33
OP_SE_GATE, OP_SE_PROJ_FIN = 34, 35
OP_SE_FC_FWD, OP_SE_FC_BWD = 37, 38
OP_STEM_DGRAD = 39
OP_BN_FROZEN_BATCH, OP_BWD_POST_FROZEN, OP_BN_BWD_FINALIZE_FROZEN = 40, 41, 42      # frozen BatchNorm statistics (include/mnas.h)
PACK_FWD, PACK_DGRAD, PACK_DW, PACK_TCONV = 0, 1, 2, 3
EINVAL = 10001      # MNAS_EINVAL
ROUTE_PWX, ROUTE_PWS, ROUTE_PWF, ROUTE_PWD, ROUTE_C3R, ROUTE_DIMG, ROUTE_C3X, ROUTE_IGEMM = range(8)     # MNAS_ROUTE_*
TCONV_TCX, TCONV_TCR, TCONV_TCONV = range(3)     # MNAS_TCONV_*


def _act(n):
    return (n + ".data", n + ".scale", n + ".shift")


def _grad(n):
    return (n + ".g", n + ".y", n + ".coef")


def _post(n):
    return tuple(n + "." + f for f in ("nsplit", "Co", "Ci", "taps", "dw", "level"))


# What run_one() (csrc/mnas_abi.hip) reads of a MnasOp, per opcode: the names of the slots of i, d and p in order (None: a retired
# slot).  THE description of the launch-list encoding: set_op() / op_field() address slots through it and nothing else spells an
# index; tests/test_abi_cpu.py holds it to run_one()'s source.  i[14] is the stream of every op (mnas_run_ops_multi).
OP_SLOTS = {
    OP_CONV_GEMM: (("mode", "N", "Hi", "Wi", "Ci", "Ho", "Wo", "Co", "kh", "kw", "stride", "pad", "nparts"), (),
                   _act("act") + _grad("grad") + ("w", "bias", "resid", "out", "stats", "red_y", "red_bn", "gate")),
    OP_CONV_WGRAD: (("N", "Hi", "Wi", "Ci", "Ho", "Wo", "Co", "kh", "kw", "stride", "pad", "nsplit"), (),
                    _act("x") + _grad("dy") + ("partial",)),
    OP_WGRAD_FINALIZE: (("nsplit", "Co", "Ci", "taps", "accumulate"), (), ("partial", "grad")),
    OP_DW_FWD: (("N", "H", "W", "C", "k", "nparts", "stride"), (), _act("in_") + ("w", "bias", "out", "stats")),
    OP_DW_BWD: (("N", "H", "W", "C", "k", "nparts", "phase", "stride", "g_masked"), (),
                _act("x") + _grad("dy") + ("w", "gin", "wpartial", "red_bn", "red_partial")),
    OP_DW_WGRAD_FINALIZE: (("nparts", "C", "k", "accumulate"), (), ("wpartial", "grad")),
    OP_STEM_FWD: (("N", "H", "W", "Ho", "Wo", "Co", "nparts", "in_u8"), (), ("x", "w", "bias", "out", "stats", "in_affine")),
    OP_STEM_WGRAD: (("N", "H", "W", "Ho", "Wo", "Co", "nparts", "in_u8"), (), ("x",) + _grad("dy") + ("partial", "in_affine")),
    OP_STEM_DGRAD: (("N", "H", "W", "Ho", "Wo", "Co"), (), _grad("dy") + ("w", "in_affine", "dx")),
    OP_BN_FWD_FINALIZE: (("nparts", "C", "training"), ("count", "momentum", "eps"),
                         ("partial", "gamma", "beta", "rmean", "rvar", "nbt", "bnbuf")),
    OP_BN_BWD_REDUCE: (("C", "nparts"), ("rows",), ("g", "y", "bnbuf", "partial")),
    OP_BN_BWD_FINALIZE: (("nparts", "C", "accumulate"), ("count",), ("partial", "bnbuf", "dgamma", "dbeta")),
    OP_ADD_ACT: (("C", "HW"), ("rows",), _act("a") + _act("b") + ("out_bf16", "out_nchw")),
    OP_NCHW_TO_NHWC: (("N", "C", "HW"), (), ("src", "dst")),
    OP_PACK_WEIGHTS: (("kind", "Co", "Ci", "kh", "kw"), (), ("w", "dst")),
    OP_PACK_BATCH: (("n",), (), ("descs",)),                   # descs: device array of MnasPackDesc
    OP_EVENT_RECORD: ((), (), ("event", "gate")),              # gate: HOST int, 0 = skip this record
    OP_EVENT_WAIT: ((), (), ("event",)),
    OP_PW_BWD: (("M", "Ci", "Co", "nparts", "gin_masked", "seg_px"), (),
                _act("x") + _grad("dy") + ("w", "resid", "gin", "wpartial", "red_partial", "red_y", "red_bn", None, "w_fwd", "b_fwd")),
    OP_POOL_ACT: (("N", "HW", "C"), (), _act("a") + ("out",)),
    OP_POOL_BWD: (("N", "HW", "C"), (), ("gpool", "g")),
    OP_DY_MAT: (("C",), ("rows",), _grad("dy") + ("out",)),
    OP_BWD_POST: (("bn_nparts", "bn_C") + _post("w1") + _post("w2"), ("count",),
                  ("bn_partial", "bnbuf", "dgamma", "dbeta", "w1.partial", "w1.grad", "w2.partial", "w2.grad")),
    OP_BWD_POST_FROZEN: (("bn_nparts", "bn_C") + _post("w1") + _post("w2"), ("count",),
                         ("bn_partial", "bnbuf", "dgamma", "dbeta", "w1.partial", "w1.grad", "w2.partial", "w2.grad", "dbias")),
    OP_BN_BWD_FINALIZE_FROZEN: (("nparts", "C", "accumulate"), (), ("partial", "bnbuf", "dgamma", "dbeta", "dbias")),
    OP_BN_FROZEN_BATCH: (("n",), (), ("descs",)),              # descs: device array of MnasBnFrozenDesc
    OP_TCONV_DGRAD: (("N", "Ho", "Wo", "Co", "Ci", "nparts"), (), ("dy", "w", "out", "stats", "red_y", "red_bn")),
    OP_HEAD_LINEAR: (("N", "I", "O", "relu", "accumulate", "which"), (),       # which: 0 forward, 1 bwd_w, 2 bwd_x; no dropout
                     ("x", "w", "b", "y", "dz", "dw", "db", "dx", "relu_mask")),
    OP_SE_SCALE: (("N", "HW", "C"), (), _act("a") + ("u", "out")),
    OP_SE_BWD_REDUCE: (("N", "HW", "C"), (), ("gs",) + _act("a") + ("u", "du", "scratch")),
    OP_SE_BWD_APPLY: (("N", "HW", "C"), (), ("gs", "u", "dz", "out", "red_y", "red_bn", "red_partial")),
    OP_SE_GATE: (("N", "C"), (), ("u", "gate")),
    OP_SE_PROJ_FIN: (("N", "kseg", "Co", "Ci", "accumulate"), (), ("wpartial", "u", "w", "grad", "du")),
    OP_SE_FC_FWD: (("N", "E", "R"), (), ("z", "w1", "b1", "w2", "b2", "hb", "u", "gate")),
    OP_SE_FC_BWD: (("N", "E", "R", "accumulate"), (), ("du", "z", "hb", "w1", "w2", "dh", "dz", "dw1", "db1", "dw2", "db2")),
}
OP_STREAM_SLOT = 14
_SLOT = {}       # opcode -> {name: ("i" | "d" | "p", index)}
_GROUP = {}      # opcode -> {prefix: [member names]}   ("x" -> x.data, x.scale, x.shift)
for _opc, _kinds in OP_SLOTS.items():
    _SLOT[_opc], _GROUP[_opc] = {}, {}
    for _kind, _names in zip("idp", _kinds):
        for _k, _name in enumerate(_names):
            if _name is None:
                continue
            if _name in _SLOT[_opc] or (_kind == "i" and _k >= OP_STREAM_SLOT):
                raise ValueError("OP_SLOTS[%d]: bad slot %s" % (_opc, _name))
            _SLOT[_opc][_name] = (_kind, _k)
            if "." in _name:
                _GROUP[_opc].setdefault(_name.split(".")[0], []).append(_name)


def slot(opcode, name):
    """index of the named slot in its array (i, d or p)"""
    return _SLOT[opcode][name][1]


def set_op(o, opcode, stream=0, **fields):
    """Fill a zeroed MnasOp by slot name (OP_SLOTS).  Pointer slots take a tensor, an address or None.  A group (x=, dy=, act=,
    w1=, ...) takes an object with act_ptrs(), a NamedTuple whose fields are the group's members, or one value per member.
    Unknown and doubly given names raise."""
    slots, oi, od, op = _SLOT[opcode], o.i, o.d, o.p
    o.opcode, oi[OP_STREAM_SLOT] = opcode, stream
    for name, v in fields.items():
        where = slots.get(name)
        if where is None:
            members = _GROUP[opcode].get(name)
            if members is None:
                raise TypeError("opcode %d: unknown slot %s" % (opcode, name))
            if hasattr(v, "_asdict"):
                v = [getattr(v, m.split(".")[1]) for m in members]
            elif hasattr(v, "act_ptrs"):
                v = v.act_ptrs()
            if len(v) != len(members) or any(m in fields for m in members):
                raise TypeError("opcode %d: group %s takes %d values, once" % (opcode, name, len(members)))
            set_op(o, opcode, stream, **dict(zip(members, v)))
            continue
        kind, k = where
        if kind == "i":
            oi[k] = v           # (ctypes converts and range-checks)
        elif kind == "d":
            od[k] = v
        else:
            op[k] = (v if v is None or type(v) is int else v.data_ptr()) or None
    return o


def op_field(o, name):
    kind, k = _SLOT[o.opcode][name]
    return getattr(o, kind)[k]


def op_ints(o):
    """the op's named integers, in slot order"""
    return tuple(int(v) for v in o.i[:len(OP_SLOTS[o.opcode][0])])


# every symbol include/mnas.h declares: (name, restype, argtypes)
class MnasHeadLinear(C.Structure):
    _fields_ = [("N", C.c_int32), ("I", C.c_int32), ("O", C.c_int32), ("relu", C.c_int32), ("accumulate", C.c_int32),
                ("drop_p", c_float), ("seed", C.c_uint64), ("x", c_void_p), ("w", c_void_p), ("b", c_void_p),
                ("y", c_void_p), ("dz", c_void_p), ("dw", c_void_p), ("db", c_void_p), ("dx", c_void_p),
                ("relu_mask", c_void_p)]


METERS_MAX_K, METERS_NUM_I64, METERS_NUM_F64 = 4, 14, 3        # MNAS_METERS_*


class MnasMeters(C.Structure):
    """include/mnas.h: 14 int64 then 3 double, every field 8 bytes wide (the block is also viewed as two tensors)"""
    _fields_ = [("steps", c_int64), ("samples", c_int64), ("loss_samples", c_int64), ("nonfinite_steps", c_int64),
                ("correct", c_int64 * 4), ("last_n", c_int64), ("last_loss_n", c_int64), ("last_correct", c_int64 * 4),
                ("loss_sum", c_double), ("last_loss", c_double), ("last_loss_sum", c_double)]


MLABEL_NUM_I64, MLABEL_NUM_F64 = 16, 9                          # MNAS_MLABEL_*


class MnasMultiLabelMeters(C.Structure):
    """include/mnas.h: 16 int64 then 9 double, every field 8 bytes wide (the block is also viewed as two tensors)"""
    _fields_ = [(n, c_int64) for n in ("steps", "samples", "nonfinite_steps", "loss_n", "dice_n", "f1_n", "tp", "fp", "fn", "last_n",
                                       "last_loss_n", "last_dice_n", "last_f1_n", "last_tp", "last_fp", "last_fn")] + \
               [(n, c_double) for n in ("loss_sum", "dice_sum", "f1_sum", "last_loss", "last_dice", "last_f1", "last_loss_sum",
                                        "last_dice_sum", "last_f1_sum")]


MLABEL_MEAN, MLABEL_ROWS = 0, 1                                 # MNAS_MLABEL_MEAN / MNAS_MLABEL_ROWS


class MnasMlabelLoss(C.Structure):
    """include/mnas.h: HOST struct of mnas_mlabel_loss's settings (32 bytes)"""
    _fields_ = [("gamma_pos", c_float), ("gamma_neg", c_float), ("margin", c_float), ("smoothing", c_float),
                ("reduction", C.c_int32), ("reserved", C.c_int32 * 3)]


GRADNORM_MAX_PARTS = 1024                                    # MNAS_GRADNORM_MAX_PARTS


class MnasGradStats(C.Structure):
    """include/mnas.h: the device block the *_step_ex launches move (32 bytes: two floats, three int64)"""
    _fields_ = [("last_norm", c_float), ("last_coef", c_float), ("steps", c_int64), ("clipped_steps", c_int64),
                ("skipped_steps", c_int64)]


class MnasOptExtra(C.Structure):
    """include/mnas.h: HOST struct of the clip / skip / EMA arguments of a *_step_ex launch"""
    _fields_ = [("partial", c_void_p), ("nparts", C.c_int32), ("max_norm", c_float), ("skip_nonfinite", C.c_int32),
                ("ema", c_void_p), ("ema_decay", c_float), ("stats", c_void_p), ("update_stats", C.c_int32)]


OPT_TILE, OPT_MAX_GROUPS, OPT_MAX_SEGS = 4096, 32, 4096          # MNAS_OPT_TILE, MNAS_OPT_MAX_GROUPS, MNAS_OPT_MAX_SEGS
TRUST_NONE, TRUST_LAMB, TRUST_LARS = 0, 1, 2                    # MNAS_TRUST_*


class MnasOptSeg(C.Structure):
    """include/mnas.h: DEVICE table entry of the *_step_seg calls, one trainable parameter tensor (32 bytes)"""
    _fields_ = [("begin", c_int64), ("n", c_int64), ("group", C.c_int32), ("tile0", C.c_int32), ("ntiles", C.c_int32),
                ("reserved", C.c_int32)]


class MnasOptTile(C.Structure):
    """include/mnas.h: DEVICE table entry, at most OPT_TILE consecutive elements of one segment (16 bytes)"""
    _fields_ = [("begin", c_int64), ("n", C.c_int32), ("seg", C.c_int32)]


class MnasOptGroup(C.Structure):
    """include/mnas.h: HOST array entry, one parameter group's scalars as they are at this step"""
    _fields_ = [("lr", c_float), ("weight_decay", c_float), ("decoupled", C.c_int32), ("trust", C.c_int32)]


class MnasOptSegs(C.Structure):
    """include/mnas.h: HOST struct of a *_step_seg call: the tables, the groups, the trust-ratio workspaces and scalars"""
    _fields_ = [("segs", c_void_p), ("tiles", c_void_p), ("groups", C.POINTER(MnasOptGroup)), ("nsegs", C.c_int32),
                ("ntiles", C.c_int32), ("ngroups", C.c_int32), ("trust_kind", C.c_int32), ("tile_partial", c_void_p),
                ("ratio", c_void_p), ("trust_coef", c_float), ("trust_eps", c_float)]


SYMBOLS = {
    "mnas_conv_img_parts": (c_int, [c_int] * 11),
    "mnas_stem_parts": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "mnas_head_linear_fwd": (c_int, [C.POINTER(MnasHeadLinear), c_void_p]),
    "mnas_head_linear_bwd_w": (c_int, [C.POINTER(MnasHeadLinear), c_void_p]),
    "mnas_head_linear_bwd_x": (c_int, [C.POINTER(MnasHeadLinear), c_void_p]),
    "mnas_head_dropout_mask": (c_int, [c_void_p, c_int64, c_float, C.c_uint64, c_void_p]),
    "mnas_head_cross_entropy": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "mnas_head_cross_entropy_metrics": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                                C.POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p]),
    "mnas_head_metrics": (c_int, [c_void_p, c_void_p, c_int, c_int, C.POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "mnas_head_cross_entropy_soft": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_int64, c_void_p,
                                             c_void_p, c_void_p, c_void_p, C.POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p]),
    "mnas_head_cross_entropy_kd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_float, c_float, c_int,
                                           c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, C.POINTER(c_int), c_int,
                                           c_void_p, c_void_p, c_void_p]),
    "mnas_mlabel_scratch_bytes": (c_int64, [c_int]),
    "mnas_mlabel_bce": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "mnas_mlabel_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, C.POINTER(MnasMlabelLoss),
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    "mnas_mlabel_metrics": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                    c_void_p]),
    "mnas_mlabel_hard_dice": (c_int, [c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p]),
    "mnas_se_scale": (c_int, [C.POINTER(MnasActIn), c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mnas_se_bwd_reduce": (c_int, [c_void_p, C.POINTER(MnasActIn), c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mnas_se_scratch_bytes": (c_int64, [c_int, c_int, c_int]),
    "mnas_se_bwd_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mnas_se_bwd_apply_cols": (c_int, [c_int, c_int, c_int]),
    "mnas_se_gate": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "mnas_se_proj_finalize": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "mnas_stem_dgrad": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p] * 3),
    "mnas_se_fc_supported": (c_int, [c_int, c_int]),
    "mnas_se_fc_fwd": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p] * 4),
    "mnas_se_fc_bwd": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p] * 6 + [c_int, c_void_p]),
    "mnas_conv_gemm_gate_ok": (c_int, [c_int, c_int, c_int, c_int]),
    "mnas_graph_create": (c_int, [C.POINTER(MnasOp), c_int, C.POINTER(c_void_p), c_int, C.POINTER(c_void_p), C.POINTER(c_int)]),
    "mnas_graph_launch": (c_int, [c_void_p, c_void_p]),
    "mnas_graph_destroy": (c_int, [c_void_p]),
    "mnas_version": (c_int, []),
    "mnas_arch": (C.c_char_p, []),
    "mnas_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "mnas_conv_gemm": (c_int, [C.POINTER(MnasConvGemm), c_void_p]),
    "mnas_conv_gemm_route": (c_int, [C.POINTER(MnasConvGemm), C.POINTER(c_int)]),
    "mnas_conv_gemm_instance": (c_int, [C.POINTER(MnasConvGemm), C.POINTER(c_int)]),
    "mnas_conv_gemm_tile_pixels": (c_int, [c_int, c_int, c_int]),
    "mnas_conv_gemm_parts": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "mnas_conv_wgrad": (c_int, [C.POINTER(MnasConvWgrad), c_void_p]),
    "mnas_conv_wgrad_instance": (c_int, [C.POINTER(MnasConvWgrad), C.POINTER(c_int)]),
    "mnas_conv_wgrad_slabs": (c_int, [c_int, c_int, c_int]),
    "mnas_wgrad_finalize": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "mnas_pw_bwd": (c_int, [C.POINTER(MnasPwBwd), c_void_p]),
    "mnas_pw_bwd_supported": (c_int, [c_int, c_int]),
    "mnas_pw_bwd_forms": (c_int, [c_int, c_int]),
    "mnas_pw_bwd_instance": (c_int, [C.POINTER(MnasPwBwd), C.POINTER(c_int)]),
    "mnas_pw_bwd_tile_pixels": (c_int, [c_int, c_int]),
    "mnas_pw_bwd_slices": (c_int, [c_int, c_int]),
    "mnas_dw_fwd": (c_int, [C.POINTER(MnasDwFwd), c_void_p]),
    "mnas_dw_bwd": (c_int, [C.POINTER(MnasDwBwd), c_void_p]),
    "mnas_dw_rows": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "mnas_dw_geometry": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_int)]),
    "mnas_dw_wgrad_finalize": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "mnas_stem_fwd": (c_int, [C.POINTER(MnasStemFwd), c_void_p]),
    "mnas_stem_wgrad": (c_int, [C.POINTER(MnasStemWgrad), c_void_p]),
    "mnas_bn_fwd_finalize": (c_int, [c_void_p, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_float, c_float, c_int, c_void_p, c_void_p]),
    "mnas_bn_bwd_reduce": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "mnas_tconv_dgrad": (c_int, [C.POINTER(MnasTconvDgrad), c_void_p]),
    "mnas_tconv_dgrad_instance": (c_int, [C.POINTER(MnasTconvDgrad), C.POINTER(c_int)]),
    "mnas_tconv_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "mnas_tconv_parts": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "mnas_bwd_post": (c_int, [C.POINTER(MnasBwdPost), c_void_p]),
    "mnas_bwd_post_frozen": (c_int, [C.POINTER(MnasBwdPostFrozen), c_void_p]),
    "mnas_bn_bwd_finalize_frozen": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "mnas_bn_frozen_tables": (c_int, [c_void_p, c_int, c_void_p]),
    "mnas_dy_materialize": (c_int, [C.POINTER(MnasGradIn), c_int64, c_int, c_void_p, c_void_p]),
    "mnas_bn_bwd_finalize": (c_int, [c_void_p, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "mnas_add_act": (c_int, [C.POINTER(MnasActIn), C.POINTER(MnasActIn), c_int64, c_int, c_void_p, c_void_p, c_int,
                             c_void_p]),
    "mnas_pool_act": (c_int, [C.POINTER(MnasActIn), c_int, c_int, c_int, c_void_p, c_void_p]),
    "mnas_pool_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mnas_nchw_f32_to_nhwc_bf16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mnas_pack_weights": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mnas_pack_weights_batch": (c_int, [c_void_p, c_int, c_void_p]),
    "mnas_packed_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "mnas_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                               c_float, c_int, c_float, c_void_p]),
    "mnas_rmsprop_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float,
                                  c_float, c_void_p]),
    "mnas_sgd_step": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_int, c_int, c_float,
                              c_void_p]),
    "mnas_grad_sqnorm": (c_int, [c_void_p, c_int64, c_float, c_void_p, c_int, C.POINTER(c_int), c_void_p]),
    "mnas_adam_step_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                                  c_float, c_int, c_float, C.POINTER(MnasOptExtra), c_void_p]),
    "mnas_rmsprop_step_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float,
                                     c_float, C.POINTER(MnasOptExtra), c_void_p]),
    "mnas_sgd_step_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_int, c_int, c_float,
                                 C.POINTER(MnasOptExtra), c_void_p]),
    "mnas_adam_step_seg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_int, c_float,
                                   C.POINTER(MnasOptSegs), C.POINTER(MnasOptExtra), c_void_p]),
    "mnas_rmsprop_step_seg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                                      C.POINTER(MnasOptSegs), C.POINTER(MnasOptExtra), c_void_p]),
    "mnas_sgd_step_seg": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, c_int, c_float,
                                  C.POINTER(MnasOptSegs), C.POINTER(MnasOptExtra), c_void_p]),
    "mnas_run_ops": (c_int, [C.POINTER(MnasOp), c_int, c_void_p, C.POINTER(c_int)]),
    "mnas_run_ops_multi": (c_int, [C.POINTER(MnasOp), c_int, C.POINTER(c_void_p), c_int, C.POINTER(c_int)]),
    "mnas_event_create": (c_int, [C.POINTER(c_void_p)]),
    "mnas_event_destroy": (c_int, [c_void_p]),
    "mnas_event_record": (c_int, [c_void_p, c_void_p]),
    "mnas_event_elapsed_ms": (c_int, [c_void_p, c_void_p, C.POINTER(c_float)]),
    "mnas_probe_copy": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "mnas_probe_valu": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "mnas_probe_copy4": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "mnas_probe_read": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "mnas_probe_empty": (c_int, [c_int, c_int, c_void_p]),
    "mnas_img_xform_check": (c_int, [C.POINTER(MnasImgXform), c_int, c_int, c_int, c_int64]),
    "mnas_img_xform": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    "mnas_img_color_check": (c_int, [C.POINTER(MnasImgColor), c_int, c_int, c_int]),
    "mnas_img_color_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "mnas_img_color": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mnas_img_mix_check": (c_int, [C.POINTER(MnasImgMix), c_int, c_int, c_int]),
    "mnas_img_mix": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mnas_img_aug_check": (c_int, [C.POINTER(MnasImgAug), c_int, c_int, c_int]),
    "mnas_img_aug_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "mnas_img_aug": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mnas_philox4x32_10": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mnas_img_erase_check": (c_int, [C.POINTER(MnasImgErase), c_int, c_int, c_int]),
    "mnas_img_erase": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, C.c_uint64, C.c_uint32, c_void_p]),
}

_lib = None


def load():
    """Load libmnas_hip.so and type every entry point.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libmnas_hip.so not built (%s): run `make -C mnasnet_pytorch_amd/csrc` or __graft_entry__.build(). "
            "There is no CPU / eager fallback for the MNASNet hot path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)     # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.mnas_version() != ABI_VERSION:
        raise RuntimeError("libmnas_hip.so ABI version %d != %d (stale build: run make -C mnasnet_pytorch_amd/csrc)" % (lib.mnas_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what="mnas call"):
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (what, rc))


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()
