"""The planning half of the engine: compiles the engine's traced steps into the static launch lists (MnasOp records, include/mnas.h)
of one (batch, height, width, mode) configuration -- one forward list and one backward list per features.<stage> segment -- and
allocates every buffer they name.  Nothing here touches a device: tensors are allocated and the library is asked host-side
questions only, so plans build (and are pinned, tests/test_launch_plan_cpu.py) on the CPU.  Slots of an op are addressed by the names
of _lib.OP_SLOTS.  engine.Program adds the run-time half."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch

from . import _lib as L

# igemm layers with fewer output pixels than this get one tile per workgroup (the 7x7 stage: 98 persistent workgroups of
# two tiles leave most of the 256 CUs idle; measured -23..-35 % per launch there, +17..+37 % on the 14x14 stage)
_SMALL_M = 20000
_STATS_PARTS = 2048          # persistent pixel-workgroups for conv kernels / rows of the stats scratch
_STEM_WGRAD_PARTS_MAX = 768  # upper bound of mnas_stem_parts(1, ...) (csrc/mnas_stem.hip): sizes the partial-slab scratch
L_BN_ROWS = 8


def _cdiv(a, b):
    return (a + b - 1) // b


def se_segments_per_image(N, HW, tile, slices, max_slabs, resident=512):
    """Workgroups per image (a divisor of HW, so that no segment straddles two images) for the segment-mode backward of a
    squeeze-excite project conv: the divisor with the least (ragged-last-tile waste) x (idle share of the last round of `resident`
    workgroups), ties to the smaller one; 0 if no divisor keeps the N*d weight-gradient slabs within `max_slabs` / 4096."""
    best = None
    for d in range(1, 65):
        if HW % d or N * d > 4096 or N * d > max_slabs:
            continue
        seg = HW // d
        waste = _cdiv(seg, tile) * tile / seg            # pixel slots per pixel (ragged last tile of a segment)
        rounds = N * d * slices / float(resident)        # two resident workgroups per CU
        cost = waste * _cdiv(N * d * slices, resident) / rounds
        if best is None or cost < best[0] - 1e-9:
            best = (cost, d)
    return best[1] if best is not None else 0


class _Act:
    """A (possibly virtual) activation: value = relu(scale*data+shift) if bn is not None else data."""
    __slots__ = ("data", "bn", "H", "W", "C", "gate")

    def __init__(self, data, bn, H, W, C_, gate=None):
        self.data, self.bn, self.H, self.W, self.C = data, bn, H, W, C_
        self.gate = gate         # squeeze-excite applied on load: fp32 [N][C] multiplier on top of the virtual activation

    def act_ptrs(self):
        if self.bn is None:
            return [self.data.data_ptr(), None, None]
        return [self.data.data_ptr(), self.bn.data_ptr(), self.bn.data_ptr() + 4 * self.C]


# one forward application of a ConvBlock (shared blocks have several); a_in None: the stem reads the image
_ConvApp = namedtuple("_ConvApp", "ci a_in out Hi Wi")
# the squeeze-excite tensors of one block application; h2: the activated depthwise output; kseg > 0: excitation applied on load,
# workgroups per image of the project conv's segment-mode backward (gate: its [N][C] table)
_SERec = namedtuple("_SERec", "se h2 z hb u kseg gate")
# kind "conv" / "block"; start: index of the step's first _ConvApp; block only: a_in, a_out = its input and its materialised sum
_Step = namedtuple("_Step", "kind stage start a_in a_out")
# a weight-gradient reduction waiting for a mnas_bwd_post launch: the fields of MnasPostWgrad
_PendWgrad = namedtuple("_PendWgrad", "partial grad nsplit Co Ci taps dw level")
# the BatchNorm-backward finalize of a mnas_bwd_post launch: the bn_* fields of MnasBwdPost
_BnPost = namedtuple("_BnPost", "bn_partial bnbuf dgamma dbeta bn_nparts bn_C count")


class _OpList:
    def __init__(self, eng, tag, stage=None):
        self.items: List[L.MnasOp] = []
        self.eng, self.tag, self.stage = eng, tag, stage

    def add(self, opcode, stream=0, **fields):
        """fields: the op's slots by name (_lib.OP_SLOTS).  stream: 0 = main (torch's current stream), 1 = the engine's side
        stream (weight-gradient work).  Returns the op's index in the list."""
        eng = self.eng
        op = L.set_op(L.MnasOp(), opcode, stream, **fields)
        prof = bool(eng.profile_opcodes) and opcode in eng.profile_opcodes
        if prof:
            ints = L.op_ints(op)
            prof = eng.profile_filter is None or eng.profile_filter(opcode, ints)
        if prof:
            ev0, ev1 = eng.new_event(), eng.new_event()
            gate = C.addressof(eng.profile_gate)          # host int: 0 = these two records are skipped (Engine.profile_gate)
            self.items.append(L.set_op(L.MnasOp(), L.OP_EVENT_RECORD, stream, event=ev0, gate=gate))
        self.items.append(op)
        idx = len(self.items) - 1
        if prof:
            self.items.append(L.set_op(L.MnasOp(), L.OP_EVENT_RECORD, stream, event=ev1, gate=gate))
            eng.profile_events.append(((self.tag, opcode, ints), ev0, ev1))
        return idx

    def fork(self):
        """side stream may start from here: it waits for everything enqueued on main so far"""
        ev = self.eng.new_event()
        self.add(L.OP_EVENT_RECORD, 0, event=ev)
        self.add(L.OP_EVENT_WAIT, 1, event=ev)

    def join(self):
        """main waits for everything enqueued on the side stream so far"""
        ev = self.eng.new_event()
        self.add(L.OP_EVENT_RECORD, 1, event=ev)
        self.add(L.OP_EVENT_WAIT, 0, event=ev)

    def build(self):
        return (L.MnasOp * max(1, len(self.items)))(*self.items), len(self.items)


class LaunchPlan:
    """All buffers + launch lists for one (N, H, W, training, need_dx) configuration.

    frozen_bn (with training): BatchNorm normalises with its RUNNING statistics and leaves them alone while every parameter still
    gets its gradient (model.train(); features.eval()).  The forward is the eval forward that keeps its activations (squeeze-excite
    blocks take the TRAINING criteria of _se_onload_kseg, since their backward has to exist: below pw_fused_min_pixels the project
    conv reads the materialised a*s where the plain eval program gates on load: the same values), with one
    mnas_bn_frozen_tables launch at its head filling every application's whole coefficient block (dy = s*dz: rows 2..4 = s, 0, 0;
    rows 5, 6 = running mean, invstd for the reduces); the backward is the train-mode list with the BatchNorm finalizes replaced by
    their frozen twins, which also accumulate the conv bias gradient s*S1 and do not write the block.

    first_trainable (with training): index into Engine.steps of the first step that owns a trainable parameter
    (Engine.first_trainable_step).  The backward ends there: the boundary step runs without its input gradient, the steps in
    front of it get no launch, the stages wholly in front of it no segment, and no buffer that only their backward needs exists.
    The forward is the same list whatever the boundary; len(steps) leaves a program without backward lists.  An input gradient
    (need_dx) needs the boundary at 0."""

    def __init__(self, eng, N, H, W, training, need_dx, pooled=False, in_u8=False, *, frozen_bn=False, first_trainable=0):
        self.eng, self.N, self.H, self.W, self.training, self.need_dx = eng, N, H, W, training, need_dx
        self.frozen_bn = bool(frozen_bn)
        if self.frozen_bn and not training:
            raise ValueError("frozen_bn is a training mode: the plain eval program is training=False")
        self.first_trainable = int(first_trainable)
        if not 0 <= self.first_trainable <= len(eng.steps):
            raise ValueError("first_trainable must be a step index in [0, %d], got %d" % (len(eng.steps), self.first_trainable))
        if self.first_trainable and (need_dx or not training):
            raise ValueError("a frozen prefix belongs to a training program without an input gradient")
        self.pooled = pooled
        self.in_u8 = bool(in_u8)
        # fused input pipeline of the stem (Engine.set_input_normalization): per-plane affine, uint8 images
        self._aff = eng.input_affine(self.in_u8)
        if self.in_u8 and self._aff is None:
            raise RuntimeError("uint8 images need Engine.set_input_normalization(mean, std)")
        self.keep = []                      # tensors owned by this program
        # what the launch lists are BUILT with (the capture decision in Program._run must not follow later changes of the engine's
        # switches: a list with stream-1 fork/join pairs or live event records cannot be captured whatever the switches say now)
        self._built_side = bool(eng.use_side_stream)
        self._built_prof = bool(eng.profile_opcodes)
        steps = self._plan_forward()
        self.bwd_segments = []      # [(stage, ops, n)]
        self.patch_gout = None      # patch_*: (stage, op index, pointer slot) receiving a run-time pointer
        self.patch_dx = None
        self.patch_x_bwd = None
        if training and self.first_trainable < len(steps):
            self._plan_backward(steps)

    # ---- forward -----------------------------------------------------------------------------------
    def _plan_forward(self):
        eng, lib, N, H, W, training = self.eng, self.eng.lib, self.N, self.H, self.W, self.training
        fwd = self._fwd = _OpList(eng, "fwd")
        # dy plane (Ho, Wo) of every stride-2 dense conv in THIS program: the transposed-conv input gradient is picked per plane
        # (rectangular clusters, 192-px inputs ... get the form whenever the library has it for their plane)
        self._tconv_ok = {}
        Ht, Wt = H, W
        for op, m, stage in eng.steps:
            for cb in ([m] if op == "conv" else m):
                ci = eng.info[id(cb)]
                Ho_, Wo_ = ci.out_hw(Ht, Wt)
                if eng.use_tconv and eng.materialize_dy and getattr(ci, "w_tconv", None) is not None and Ht == 2 * Ho_ and Wt == 2 * Wo_:
                    self._tconv_ok[id(ci)] = bool(lib.mnas_tconv_supported(Ho_, Wo_, ci.cout, ci.cin)) and \
                        lib.mnas_tconv_parts(N, Ho_, Wo_, ci.cout, ci.cin) > 0
                Ht, Wt = Ho_, Wo_
        # ---- weight packing (once per forward; weights change every optimizer step): one batched launch
        descs = []
        for ci in eng.convs:
            w = ci.mod.conv.weight
            if ci.kind in ("pw", "dense"):
                descs.append((w.data_ptr(), ci.w_fwd.data_ptr(), L.PACK_FWD, ci.cout, ci.cin, ci.k * ci.k))
                if training:
                    descs.append((w.data_ptr(), ci.w_dgrad.data_ptr(), L.PACK_DGRAD, ci.cout, ci.cin, ci.k * ci.k))
                    if self._tconv_ok.get(id(ci)):
                        descs.append((w.data_ptr(), ci.w_tconv.data_ptr(), L.PACK_TCONV, ci.cout, ci.cin, 9))
            elif ci.kind == "dw":
                descs.append((w.data_ptr(), ci.w_fwd.data_ptr(), L.PACK_DW, ci.cout, 1, ci.k * ci.k))
            else:  # stem: [Co][27] viewed as a 1x1 conv over 27 "channels"
                descs.append((w.data_ptr(), ci.w_fwd.data_ptr(), L.PACK_FWD, ci.cout, 27, 1))
        host = (L.MnasPackDesc * len(descs))(*descs)
        raw = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(eng.device)
        self.keep.append(raw)
        fwd.add(L.OP_PACK_BATCH, n=len(descs), descs=raw)
        # frozen statistics: every application's coefficient block in one launch; its descriptor table is filled in below, once the
        # blocks exist
        j_frozen = fwd.add(L.OP_BN_FROZEN_BATCH, n=0) if self.frozen_bn else None

        self.x_is_image = eng.first_conv.kind == "stem"
        self.patch_x = []       # (op index, pointer slot) receiving the input pointer
        self._records: List[_ConvApp] = []      # forward applications, for the backward builder
        Hc, Wc = H, W
        if self.x_is_image:
            cur = None          # the stem reads the fp32 NCHW input directly
        else:
            Cin = eng.first_conv.cin
            xb = self._new((N, H, W, Cin))
            j = fwd.add(L.OP_NCHW_TO_NHWC, N=N, C=Cin, HW=H * W, dst=xb)
            self.patch_x.append((j, L.slot(L.OP_NCHW_TO_NHWC, "src")))
            cur = _Act(xb, None, H, W, Cin)
        self.in_channels = 3 if self.x_is_image else cur.C
        self._se_records: Dict[int, _SERec] = {}    # record index of a project conv -> its block's squeeze-excite tensors
        steps = []
        for op, m, stage in eng.steps:
            start = len(self._records)
            if op == "conv":
                cur = self._conv_fwd(eng.info[id(m)], cur, Hc, Wc)
                Hc, Wc = cur.H, cur.W
                steps.append(_Step("conv", stage, start, None, None))
            else:
                a_in = cur
                se = eng.se_info.get(id(m[0]))
                h = cur
                for j_, cb in enumerate(m):
                    ci_ = eng.info[id(cb)]
                    if j_ == 2 and se is not None:
                        h = self._se_fwd(se, h, Hc, Wc, ci_)
                    h = self._conv_fwd(ci_, h, Hc, Wc)
                r = self._new((N, Hc, Wc, a_in.C))
                fwd.add(L.OP_ADD_ACT, C=a_in.C, HW=Hc * Wc, rows=N * Hc * Wc, a=a_in, b=h, out_bf16=r)
                cur = _Act(r, None, Hc, Wc, a_in.C)
                steps.append(_Step("block", stage, start, a_in, cur))
        # ---- features output: fp32 NCHW (classifiers.py:109 consumes it), or, pooled, its global average [N][C]
        # (AdaptiveAvgPool2d(1) fused with the last BatchNorm+ReLU: the feature map is never written)
        if self.pooled:
            self.out_shape = (N, cur.C)
            j = fwd.add(L.OP_POOL_ACT, N=N, HW=cur.H * cur.W, C=cur.C, a=cur)
            self.patch_out = (j, L.slot(L.OP_POOL_ACT, "out"))
        else:
            self.out_shape = (N, cur.C, cur.H, cur.W)
            j = fwd.add(L.OP_ADD_ACT, C=cur.C, HW=cur.H * cur.W, rows=N * cur.H * cur.W, a=cur)
            self.patch_out = (j, L.slot(L.OP_ADD_ACT, "out_nchw"))
        if self.frozen_bn:
            fdescs = []
            for rec in self._records:
                bnm = rec.ci.mod.bn
                fdescs.append((bnm.weight.data_ptr(), bnm.bias.data_ptr(), bnm.running_mean.data_ptr(), bnm.running_var.data_ptr(),
                               rec.out.bn.data_ptr(), rec.ci.cout, bnm.eps))
            host = (L.MnasBnFrozenDesc * len(fdescs))(*fdescs)
            raw = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(eng.device)
            self.keep.append(raw)
            L.set_op(fwd.items[j_frozen], L.OP_BN_FROZEN_BATCH, 0, n=len(fdescs), descs=raw)
        self.fwd_ops, self.fwd_n = fwd.build()
        self.final = cur
        return steps

    def _new(self, shape, dtype=torch.bfloat16):
        t = torch.empty(shape, dtype=dtype, device=self.eng.device)
        self.keep.append(t)
        return t

    def _bnbuf(self, C_):
        t = torch.zeros((L_BN_ROWS, C_), dtype=torch.float32, device=self.eng.device)
        self.keep.append(t)
        return t

    def _igemm_tiles(self, M, Cin, Cout, taps, cap):
        """persistent pixel-workgroups of a k_igemm launch the library names no grid for"""
        return max(1, min(cap, _cdiv(M, 128 if M >= _SMALL_M else self.eng.lib.mnas_conv_gemm_tile_pixels(M, Cout, taps * Cin))))

    def _igemm_parts(self, mode, M, Cin, Cout, taps, cap):
        nparts = self.eng.lib.mnas_conv_gemm_parts(mode, M, Cin, Cout, taps)
        return nparts if nparts >= 1 else self._igemm_tiles(M, Cin, Cout, taps, cap)

    @staticmethod
    def _dw_parts(M, C_, cap):
        """persistent workgroups of a depthwise launch"""
        return max(64, min(cap, _cdiv(M * C_, 256 * 16 * 2)))

    def _conv_fwd(self, ci, a_in: Optional[_Act], Hi, Wi):
        eng, lib, N, training, fwd = self.eng, self.eng.lib, self.N, self.training, self._fwd
        Ho, Wo = ci.out_hw(Hi, Wi)
        M = N * Ho * Wo
        y = self._new((N, Ho, Wo, ci.cout))
        bn = self._bnbuf(ci.cout)
        conv, bnm = ci.mod.conv, ci.mod.bn
        stats = eng.scratch_stats if (training and not self.frozen_bn) else None      # no statistics partials from running buffers
        if ci.kind == "stem":
            nparts = lib.mnas_stem_parts(0, N, Hi, Wi, ci.cout)
            if self._aff is not None and (nparts < 1 or (training and lib.mnas_stem_parts(1, N, Hi, Wi, ci.cout) < 1)):
                # the fused Normalize / uint8 load exists only in the band kernels (csrc/mnas_stem.hip)
                raise NotImplementedError(
                    "fused input normalisation needs the stem band kernels: 32 output channels and an image width that is a "
                    "multiple of 4 (16 in training); got %dx%d, %d channels.  Normalise on the host or call "
                    "set_input_normalization(None, None)" % (Hi, Wi, ci.cout))
            if nparts < 1:
                nparts = self._igemm_tiles(M, ci.cin, ci.cout, ci.k * ci.k, eng.igemm_fwd_parts)
            j = fwd.add(L.OP_STEM_FWD, N=N, H=Hi, W=Wi, Ho=Ho, Wo=Wo, Co=ci.cout, nparts=nparts, in_u8=self.in_u8,
                        w=ci.w_fwd, bias=conv.bias, out=y, stats=stats, in_affine=self._aff)
            self.patch_x.append((j, L.slot(L.OP_STEM_FWD, "x")))
        elif ci.kind == "dw":
            nlaunch = self._dw_parts(M, ci.cout, _STATS_PARTS)
            # stride 2 = SepConv(reduce=True)'s depthwise conv (mnasnet.py:73-81): plain direct kernels (csrc/mnas_dw2.hip)
            fwd.add(L.OP_DW_FWD, N=N, H=Hi, W=Wi, C=ci.cout, k=ci.k, nparts=nlaunch, stride=ci.stride,
                    in_=a_in, w=ci.w_fwd, bias=conv.bias, out=y, stats=stats)
            nparts = lib.mnas_dw_rows(N, Hi, Wi, ci.cout, ci.k, nlaunch, 0 if ci.stride == 1 else 4)      # columns of the stats table
            if nparts < 1:
                raise RuntimeError("unsupported depthwise shape %s" % ((N, Hi, Wi, ci.cout, ci.k),))
        else:
            nparts = self._igemm_parts(0, M, ci.cin, ci.cout, ci.k * ci.k, eng.igemm_fwd_parts)
            if ci.kind == "dense":       # small maps: one image per workgroup (csrc/mnas_dimg.hip)
                ip = lib.mnas_conv_img_parts(0, N, Hi, Wi, ci.cin, Ho, Wo, ci.cout, ci.k, ci.stride, ci.pad)
                nparts = ip if ip > 0 else nparts
            fwd.add(L.OP_CONV_GEMM, mode=0, N=N, Hi=Hi, Wi=Wi, Ci=ci.cin, Ho=Ho, Wo=Wo, Co=ci.cout, kh=ci.k, kw=ci.k,
                    stride=ci.stride, pad=ci.pad, nparts=nparts, act=a_in, w=ci.w_fwd, bias=conv.bias, out=y, stats=stats,
                    gate=a_in.gate)
        if not self.frozen_bn:       # (frozen: OP_BN_FROZEN_BATCH at the head of the list wrote the block)
            fwd.add(L.OP_BN_FWD_FINALIZE, nparts=nparts, C=ci.cout, training=training, count=M, momentum=bnm.momentum, eps=bnm.eps,
                    partial=stats, gamma=bnm.weight, beta=bnm.bias, rmean=bnm.running_mean, rvar=bnm.running_var,
                    nbt=bnm.num_batches_tracked, bnbuf=bn)
        out = _Act(y, bn, Ho, Wo, ci.cout)
        self._records.append(_ConvApp(ci, a_in, out, Hi, Wi))
        return out

    def _se_onload_kseg(self, p_ci, h2: _Act, Hi, Wi):
        """Workgroups per image of the project conv's segment-mode backward when the excitation can be applied ON LOAD for this
        block (Engine.se_on_load): forward = MnasConvGemm.gate, backward = mnas_pw_bwd on the ungated activation with
        per-image weight-gradient slabs + mnas_se_proj_finalize.  0: keep the materialised a*s (k_se_scale) path."""
        eng, lib, N = self.eng, self.eng.lib, self.N
        HW, M, Ci, Co = Hi * Wi, self.N * Hi * Wi, p_ci.cin, p_ci.cout
        if not eng.se_on_load or h2.bn is None or p_ci.kind != "pw" or not lib.mnas_conv_gemm_gate_ok(N, HW, Ci, Co):
            return 0
        if not self.training:
            return 1
        # (a frozen_bn program is a training program: where these criteria fail its forward materialises a*s while the plain eval
        # forward gates on load; the values are the same either way)
        if M < eng.pw_fused_min_pixels or not lib.mnas_pw_bwd_supported(Ci, Co):
            return 0
        tile, slices = lib.mnas_pw_bwd_tile_pixels(Ci, Co), lib.mnas_pw_bwd_slices(Ci, Co)
        return se_segments_per_image(N, HW, tile, slices, eng.scratch_wgrad2.numel() // (Co * Ci))

    def _se_fwd(self, se, h2: _Act, Hi, Wi, p_ci):
        """squeeze-excite on the activated depthwise output (csrc/mnas_se.hip): pooled mean -> fc1+ReLU -> fc2 -> a2 * sigmoid.
        Returns what the project conv reads: the MATERIALISED scaled activation, or (Engine.se_on_load, supported shapes) the
        virtual activation with the excitation as a per-(image, channel) gate applied on load."""
        eng, lib, N, fwd = self.eng, self.eng.lib, self.N, self._fwd
        E_, R_ = se.channels, se.reduced
        z = self._new((N, E_), torch.float32)
        hb = self._new((N, R_), torch.float32)
        u = self._new((N, E_), torch.float32)
        fc1, fc2 = se.mod.fc1, se.mod.fc2
        fwd.add(L.OP_POOL_ACT, N=N, HW=Hi * Wi, C=E_, a=h2, out=z)
        kseg = self._se_onload_kseg(p_ci, h2, Hi, Wi)
        gate = self._new((N, E_), torch.float32) if kseg else None
        if eng.se_fused_mlp and lib.mnas_se_fc_supported(E_, R_):
            # the whole excitation MLP (+ the gate table) in one launch (csrc/mnas_se.hip k_se_fc_fwd)
            fwd.add(L.OP_SE_FC_FWD, N=N, E=E_, R=R_, z=z, w1=fc1.weight, b1=fc1.bias, w2=fc2.weight, b2=fc2.bias, hb=hb, u=u, gate=gate)
        else:
            fwd.add(L.OP_HEAD_LINEAR, N=N, I=E_, O=R_, relu=1, accumulate=0, which=0, x=z, w=fc1.weight, b=fc1.bias, y=hb)
            fwd.add(L.OP_HEAD_LINEAR, N=N, I=R_, O=E_, relu=0, accumulate=0, which=0, x=hb, w=fc2.weight, b=fc2.bias, y=u)
            if kseg:
                fwd.add(L.OP_SE_GATE, N=N, C=E_, u=u, gate=gate)
        self._se_records[len(self._records)] = _SERec(se, h2, z, hb, u, kseg, gate)    # keyed by the record index of the project conv that follows
        if kseg:
            return _Act(h2.data, h2.bn, Hi, Wi, E_, gate)
        a2s = self._new((N, Hi, Wi, E_))
        fwd.add(L.OP_SE_SCALE, N=N, HW=Hi * Wi, C=E_, a=h2, u=u, out=a2s)
        return _Act(a2s, None, Hi, Wi, E_)

    # ---- backward ----------------------------------------------------------------------------------
    def _plan_backward(self, steps: List[_Step]):
        """The backward launch lists, one per features.<stage> segment, from the forward's records (reverse order), down to the
        boundary step self.first_trainable."""
        eng, N, H, W, need_dx, records, cur = self.eng, self.N, self.H, self.W, self.need_dx, self._records, self.final
        first = self.first_trainable
        self._seg_ops: Dict[int, _OpList] = {}
        self._order: List[int] = []
        last = self._seg(steps[-1].stage)
        g_final = self._new((N, cur.H, cur.W, cur.C))
        if self.pooled:
            j = last.add(L.OP_POOL_BWD, N=N, HW=cur.H * cur.W, C=cur.C, g=g_final)
            self.patch_gout = (last.stage, j, L.slot(L.OP_POOL_BWD, "gpool"))
        else:
            j = last.add(L.OP_NCHW_TO_NHWC, N=N, C=cur.C, HW=cur.H * cur.W, dst=g_final)
            self.patch_gout = (last.stage, j, L.slot(L.OP_NCHW_TO_NHWC, "src"))

        # ---- merged bookkeeping launches (mnas_bwd_post): the weight-gradient reductions of the main-stream kernel that just
        # ran ride in the SAME launch as the next layer's BatchNorm-backward finalize (and the second level of a two-level
        # reduction in the one after that), instead of 2-3 tiny dependent launches in every gap of the main stream
        self._pend = SimpleNamespace(w1=None, w2=None, ops=None)     # reductions queued for the next mnas_bwd_post launches, and the list the last went to
        self._rot = 0
        self._rot_bufs = [eng.scratch_wgrad2, eng.scratch_wgrad3, eng.scratch_wgrad4]
        self._masked_g = set()       # data_ptr of gradient tensors stored masked (dz) by their producer
        # the record of a conv step that ends the backward: its depthwise sweep runs without the fused reduce, the one form that
        # takes no masked gradient (_feeds_fused_dw)
        self._end_rec = records[steps[first].start] if not (first == 0 and need_dx) else None
        g = g_final
        g_red = 0            # number of fused-reduce partial columns already written for the layer g belongs to
        for si in range(len(steps) - 1, first - 1, -1):
            step = steps[si]
            ops = self._seg(step.stage)
            need = si > first or (need_dx and first == 0)     # does anybody want the gradient of the step's input
            if step.kind == "conv":
                rec = records[step.start]
                g, g_red = self._conv_bwd(ops, rec, g, None, need, g_red, self._input_target(steps, si, rec.a_in))
            else:
                re_, rd, rp = records[step.start:step.start + 3]
                G = g                                   # grad wrt the block output (materialised sum)
                se_rec = self._se_records.get(step.start + 2)
                if se_rec is not None and se_rec.kseg:
                    # excitation on load: the project conv's backward runs on the UNGATED activation in segment mode; its
                    # weight-gradient slabs give du and (gated) dW3 without a pass over gs / a2 (csrc/mnas_se.hip)
                    gs_, du_ = self._conv_bwd_se_proj(ops, rp, G, g_red, se_rec)
                    g2, c2 = self._se_bwd(ops, se_rec, gs_, du_)
                else:
                    g2, c2 = self._conv_bwd(ops, rp, G, None, True, g_red, self._target_of(rp.a_in))
                    if se_rec is not None:
                        g2, c2 = self._se_bwd(ops, se_rec, g2)         # g2 becomes dL/d(activated depthwise output)
                g1, c1 = self._conv_bwd(ops, rd, g2, None, True, c2, self._target_of(rd.a_in))
                if need:
                    # expand dgrad (+ skip gradient fused in its epilogue) produces the gradient of the block INPUT:
                    # either a virtual activation (producer conv) or the previous block's sum (-> its project conv)
                    g, g_red = self._conv_bwd(ops, re_, g1, G, True, c1, self._input_target(steps, si, step.a_in))
                else:
                    self._conv_bwd(ops, re_, g1, None, False, c1, None)
                    g, g_red = None, 0
        if need_dx and not self.x_is_image:
            seg0 = self._seg(steps[0].stage)
            j = seg0.add(L.OP_ADD_ACT, C=self.in_channels, HW=H * W, rows=N * H * W, a=(g, None, None))
            self.patch_dx = (seg0.stage, j, L.slot(L.OP_ADD_ACT, "out_nchw"))
        self._flush_post()
        order, built = self._order, {}
        for st in order:
            # the main stream waits for the side stream's weight gradients at the end of backward, and at the end of the
            # stages somebody consumes right away (Trainer: the stage that completes gradient bucket 0); joining after every
            # stage cost 0.1 ms/step of main-stream waits with nobody looking at the gradients
            if eng.join_stages is None:
                need = st == order[-1] or eng.on_stage_done is not None
            else:
                need = st == order[-1] or st in eng.join_stages
            if eng.use_side_stream and need:
                self._seg_ops[st].join()
            built[st] = self._seg_ops[st].build()
        self.bwd_segments = [(st,) + built[st] for st in order]
        self._seg_index = {st: n for n, st in enumerate(order)}
        # all segments as ONE list (graph mode without a stage-done callback: one hipGraphLaunch per backward instead of one per
        # stage -- every graph boundary is ~9 us of idle GPU)
        n_all = sum(built[st][1] for st in order)
        self.bwd_all = (L.MnasOp * max(1, n_all))()
        self.bwd_all_n, self._seg_off, k = n_all, {}, 0
        for st in order:
            arr, n = built[st]
            self._seg_off[st] = k
            C.memmove(C.byref(self.bwd_all, k * C.sizeof(L.MnasOp)), arr, n * C.sizeof(L.MnasOp))
            k += n

    def _seg(self, stage) -> _OpList:
        if stage not in self._seg_ops:
            self._seg_ops[stage] = _OpList(self.eng, "bwd", stage)
            self._order.append(stage)
        return self._seg_ops[stage]

    @staticmethod
    def _target_of(act: Optional[_Act]):
        """(raw y tensor, bnbuf) of the ConvBlock that produced a VIRTUAL activation, else None."""
        if act is None or act.bn is None:
            return None
        return (act.data, act.bn)

    def _input_target(self, steps, si, a_in: Optional[_Act]):
        """Whose BatchNorm backward the gradient of step si's input feeds: the ConvBlock behind a virtual activation, or, when the
        input is the previous block's materialised sum, that block's project conv; None for the network input."""
        if a_in is not None and a_in.bn is None and si > 0 and steps[si - 1].kind == "block":
            return self._target_of(self._records[steps[si - 1].start + 2].out)
        return self._target_of(a_in)

    def _next_scratch(self):
        b = self._rot_bufs[self._rot % 3]
        self._rot += 1
        return b

    def _emit_post(self, ops: _OpList, bn=None, dbias=None):
        """dbias (frozen statistics only): the conv bias gradient slice of the ConvBlock `bn` belongs to"""
        pend = self._pend
        w1, w2 = pend.w1, pend.w2
        pend.w1 = pend.w2 = None
        if w1 is not None and w1.level == 2:
            pend.w2 = w1._replace(level=3)
        fields = {} if bn is None else bn._asdict()
        if bn is not None and self.frozen_bn:
            fields["dbias"] = dbias
        if w1 is not None:
            fields["w1"] = w1
        if w2 is not None:
            fields["w2"] = w2
        if not fields:
            return
        # frozen statistics: the twin that leaves bnbuf alone (a launch without a BatchNorm part stays mnas_bwd_post)
        ops.add(L.OP_BWD_POST_FROZEN if (bn is not None and self.frozen_bn) else L.OP_BWD_POST, **fields)
        pend.ops = ops

    def _flush_post(self):
        pend = self._pend
        while pend.w1 is not None or pend.w2 is not None:
            self._emit_post(pend.ops)

    def _queue_wgrad(self, ops, partial, nsplit, Co_, Ci_, taps, dw, grad_ptr):
        self._pend.w1 = _PendWgrad(partial, grad_ptr, nsplit, Co_, Ci_, taps, 1 if dw else 0, 1 if nsplit <= 256 else 2)
        self._pend.ops = ops

    def _bn_bwd(self, ops: _OpList, rec, g, g_reduced):
        """The BatchNorm backward in front of a ConvBlock application's conv backward: the reduce over (g, y) unless the producer
        of g already wrote its `g_reduced` partial columns into eng.scratch_red (fused epilogue), then the finalize -- merged with
        the pending weight-gradient reductions (Engine.merge_post) or a launch of its own.  Returns the dy triple (g, y, coefficients)."""
        eng, ci, out = self.eng, rec.ci, rec.out
        Co, M = ci.cout, self.N * out.H * out.W
        if g_reduced:
            nred, red_buf = g_reduced, eng.scratch_red
        else:
            nred = max(1, min(1024, _cdiv(M * Co, 256 * 8 * 8)))
            red_buf = eng.scratch_stats
            ops.add(L.OP_BN_BWD_REDUCE, C=Co, nparts=nred, rows=M, g=g, y=out.data, bnbuf=out.bn, partial=red_buf)
        if eng.merge_post:
            if self._pend.ops is not None and self._pend.ops is not ops:
                self._flush_post()               # a stage's gradients are complete inside its own launch list
            self._emit_post(ops, _BnPost(red_buf, out.bn, eng.gptr(ci, 2), eng.gptr(ci, 3), nred, Co, float(M)), eng.gptr(ci, 1))
        elif self.frozen_bn:
            ops.add(L.OP_BN_BWD_FINALIZE_FROZEN, nparts=nred, C=Co, accumulate=1,
                    partial=red_buf, bnbuf=out.bn, dgamma=eng.gptr(ci, 2), dbeta=eng.gptr(ci, 3), dbias=eng.gptr(ci, 1))
        else:
            ops.add(L.OP_BN_BWD_FINALIZE, nparts=nred, C=Co, accumulate=1, count=M,
                    partial=red_buf, bnbuf=out.bn, dgamma=eng.gptr(ci, 2), dbeta=eng.gptr(ci, 3))
        return (g, out.data, out.bn)

    def _conv_bwd(self, ops: _OpList, rec, g, resid, need_gin, g_reduced, red_target):
        """Backward of one ConvBlock application.  g: bf16 grad wrt its activated output.
        g_reduced: the producer of g already wrote this layer's BN-backward partial sums into
        eng.scratch_red (fused epilogue) with `g_reduced` columns (0: nobody did).  red_target: (y, bn) of the ConvBlock
        whose activated output is THIS layer's input -- the dgrad epilogue then does that reduce.
        Returns (gin, ncols) : bf16 grad wrt the (activated) input or None, and the number of partial
        columns written for red_target (0 if not fused)."""
        eng, lib, ci = self.eng, self.eng.lib, rec.ci
        Co, M = ci.cout, self.N * rec.out.H * rec.out.W
        if ci.kind == "dw" and resid is not None:
            raise AssertionError("residual add into a depthwise dgrad does not occur")
        gy = self._bn_bwd(ops, rec, g, g_reduced)
        # the weight-gradient kernels only share READ-ONLY inputs (g, y, the dy coefficients just finalised, the
        # forward activations) with the input-gradient chain: with Engine.use_side_stream they go to the side stream
        dyb = None
        if ci.kind == "dense" and eng.materialize_dy:
            # dense 3x3: every dy element is gathered 2.25-10 times by the input/weight-gradient kernels; form it once
            dyb = self._new((self.N, rec.out.H, rec.out.W, Co))
            ops.add(L.OP_DY_MAT, C=Co, rows=M, dy=gy, out=dyb)
        WS = 1 if (eng.use_side_stream and M <= eng.side_stream_max_pixels) else 0
        if WS:
            ops.fork()
        rt = red_target if need_gin else None
        if ci.kind == "stem":
            return self._bwd_stem(ops, rec, gy, need_gin, WS)
        if ci.kind == "dw" and ci.stride == 2:
            return self._bwd_dw_stride2(ops, rec, g, gy, need_gin, WS)
        if ci.kind == "dw":
            return self._bwd_dw(ops, rec, g, gy, rt, WS)
        if (ci.kind == "pw" and need_gin and M >= eng.pw_fused_min_pixels and lib.mnas_pw_bwd_supported(ci.cin, Co)
                and not (M < eng.pw_split_max_pixels and resid is None and Co < ci.cin and Co <= 128
                         and lib.mnas_conv_gemm_parts(1, M, Co, ci.cin, 1) > 0)):
            return self._bwd_pw_fused(ops, rec, gy, resid, rt)
        return self._bwd_gemm(ops, rec, gy, dyb, resid, need_gin, rt, WS)

    def _bwd_stem(self, ops, rec, gy, need_gin, WS):
        eng, lib, N, ci, Hi, Wi = self.eng, self.eng.lib, self.N, rec.ci, rec.Hi, rec.Wi
        Ho, Wo, Co = rec.out.H, rec.out.W, ci.cout
        nsp = max(1, min(512, _cdiv(N * Ho * Wo, 1024)))
        sp = lib.mnas_stem_parts(1, N, Hi, Wi, Co)
        nsp = min(sp if sp > 0 else nsp, _STEM_WGRAD_PARTS_MAX)
        if nsp * Co * 27 > eng.scratch_wgrad.numel():
            raise RuntimeError("stem weight-gradient scratch too small (%d splits)" % nsp)
        jx = ops.add(L.OP_STEM_WGRAD, WS, N=N, H=Hi, W=Wi, Ho=Ho, Wo=Wo, Co=Co, nparts=nsp, in_u8=self.in_u8,
                     dy=gy, partial=eng.scratch_wgrad, in_affine=self._aff)
        self.patch_x_bwd = (ops.stage, jx, L.slot(L.OP_STEM_WGRAD, "x"))
        ops.add(L.OP_WGRAD_FINALIZE, WS, nsplit=nsp, Co=Co, Ci=27, taps=1, accumulate=1, partial=eng.scratch_wgrad, grad=eng.gptr(ci, 0))
        if need_gin:
            # dL/d image (fp32 NCHW; csrc/mnas_stem.hip k_stem_dgrad): not on the training path, autograd completeness only
            if self.in_u8:
                raise RuntimeError("a uint8 image has no gradient")
            jd = ops.add(L.OP_STEM_DGRAD, N=N, H=Hi, W=Wi, Ho=Ho, Wo=Wo, Co=Co, dy=gy, w=ci.mod.conv.weight, in_affine=self._aff)
            self.patch_dx = (ops.stage, jd, L.slot(L.OP_STEM_DGRAD, "dx"))
        return None, 0

    def _bwd_dw_stride2(self, ops, rec, g, gy, need_gin, WS):
        # SepConv(reduce=True): two plain launches, no fused reduce (the producer of x runs its own mnas_bn_bwd_reduce)
        eng, N, ci, Hi, Wi, Co = self.eng, self.N, rec.ci, rec.Hi, rec.Wi, rec.ci.cout
        nparts = self._dw_parts(N * rec.out.H * rec.out.W, Co, eng.dw_bwd_parts)
        if g.data_ptr() in self._masked_g:
            raise AssertionError("masked gradient handed to the stride-2 depthwise backward")
        wrows = eng.lib.mnas_dw_rows(N, Hi, Wi, Co, ci.k, nparts, 7)
        if wrows < 1 or wrows * ci.k * ci.k * Co > eng.scratch_wgrad.numel():
            raise RuntimeError("unsupported stride-2 depthwise shape %s" % ((N, Hi, Wi, Co, ci.k),))
        geom = dict(N=N, H=Hi, W=Wi, C=Co, k=ci.k, nparts=nparts, stride=2, g_masked=0, x=rec.a_in, dy=gy, w=ci.w_fwd)
        ops.add(L.OP_DW_BWD, WS, phase=2, wpartial=eng.scratch_wgrad, **geom)              # weight gradient
        ops.add(L.OP_DW_WGRAD_FINALIZE, WS, nparts=wrows, C=Co, k=ci.k, accumulate=1, wpartial=eng.scratch_wgrad, grad=eng.gptr(ci, 0))
        gin = None
        if need_gin:
            gin = self._new((N, Hi, Wi, ci.cin))
            ops.add(L.OP_DW_BWD, phase=1, gin=gin, **geom)           # input gradient
        return gin, 0

    def _bwd_dw(self, ops, rec, g, gy, rt, WS):
        eng, lib, N, ci, Hi, Wi, Co = self.eng, self.eng.lib, self.N, rec.ci, rec.Hi, rec.Wi, rec.ci.cout
        merge, fused = eng.merge_post, ci.k in eng.dw_fused_k
        nparts = self._dw_parts(N * rec.out.H * rec.out.W, Co, eng.dw_bwd_parts)
        gin = self._new((N, Hi, Wi, ci.cin))
        ncols = 0
        wsc = (self._next_scratch() if merge else eng.scratch_wgrad2) if fused else eng.scratch_wgrad     # fused: main stream
        geom = dict(N=N, H=Hi, W=Wi, C=Co, k=ci.k, nparts=nparts, x=rec.a_in, dy=gy, w=ci.w_fwd, gin=gin, wpartial=wsc)
        if rt is not None:
            geom.update(red_bn=rt[1], red_partial=eng.scratch_red)
            ncols = lib.mnas_dw_rows(N, Hi, Wi, Co, ci.k, nparts, 1 if fused else 2)
        wrows = lib.mnas_dw_rows(N, Hi, Wi, Co, ci.k, nparts, 1 if fused else 3)
        if wrows < 1 or (rt is not None and ncols < 1):
            raise RuntimeError("unsupported depthwise shape %s" % ((N, Hi, Wi, Co, ci.k),))
        if fused:
            # one sweep: dgrad + wgrad (+ fused reduce); both partial tables have `wrows` rows
            if rt is not None:
                ncols = wrows
            # g written by a project conv's out-stage backward as dz = g*[s*y+t>0] (see _bwd_pw_fused): dy-on-read skips the mask
            gm = 1 if g.data_ptr() in self._masked_g else 0
            if gm and rt is None:
                raise AssertionError("masked gradient handed to a depthwise backward without the fused reduce")
            ops.add(L.OP_DW_BWD, phase=0, stride=0, g_masked=gm, **geom)
            if merge:
                self._queue_wgrad(ops, wsc, wrows, Co, 1, ci.k * ci.k, True, eng.gptr(ci, 0))
            else:
                ops.add(L.OP_DW_WGRAD_FINALIZE, nparts=wrows, C=Co, k=ci.k, accumulate=1, wpartial=eng.scratch_wgrad2, grad=eng.gptr(ci, 0))
        else:
            if g.data_ptr() in self._masked_g:
                raise AssertionError("masked gradient handed to the two-launch depthwise backward")
            ops.add(L.OP_DW_BWD, WS, phase=2, **geom)          # weight gradient
            ops.add(L.OP_DW_WGRAD_FINALIZE, WS, nparts=wrows, C=Co, k=ci.k, accumulate=1, wpartial=eng.scratch_wgrad, grad=eng.gptr(ci, 0))
            ops.add(L.OP_DW_BWD, phase=1, **geom)           # input gradient
        return gin, ncols

    def _bwd_pw_fused(self, ops, rec, gy, resid, rt):
        # large-pixel-count 1x1 conv: ONE sweep produces the input gradient, the weight-gradient partials and the
        # fused reduce (both former kernels stream the same g, y; see csrc/mnas_pwbwd.hip).  Main stream.
        eng, lib, N, ci, a_in, Co = self.eng, self.eng.lib, self.N, rec.ci, rec.a_in, rec.ci.cout
        M = N * rec.out.H * rec.out.W
        forms = lib.mnas_pw_bwd_forms(ci.cin, Co)
        gin = self._new((N, rec.Hi, rec.Wi, ci.cin))
        nparts = max(1, min(eng.pw_bwd_parts_large if M >= 800000 else (eng.pw_bwd_parts_mid if M >= 100000 else eng.pw_bwd_parts_small),
                            _cdiv(M, 128 if max(ci.cin, Co) <= 80 else 64)))
        wsc = self._next_scratch() if eng.merge_post else eng.scratch_wgrad2
        fields = dict(x=a_in, dy=gy, w=ci.w_dgrad, resid=resid, gin=gin, wpartial=wsc)
        if rt is not None:
            fields.update(red_partial=eng.scratch_red, red_y=rt[0], red_bn=rt[1])
        if eng.pw_recompute_y and (forms & 2):
            # widening (expand) conv: dy-on-load's raw forward output is recomputed from the staged x tile on the matrix
            # cores (bit-identical to the stored tensor) instead of being read: a third of the launch's reads
            fields.update(dy=(gy[0], None, gy[2]), w_fwd=ci.w_fwd, b_fwd=ci.mod.conv.bias)
        # project conv in front of a depthwise conv: the out-stage form stores the input gradient already masked with the
        # depthwise conv's ReLU (the mask its fused reduce computes anyway); mnas_dw_bwd then skips re-deriving it per window column
        masked = 0
        if (eng.dw_masked_g and rt is not None and resid is None and a_in.bn is not None and rt[0] is a_in.data
                and (forms & 4) and self._feeds_fused_dw(a_in)):
            masked = 1
            self._masked_g.add(gin.data_ptr())
        seg = 0
        if eng.pw_bwd_segments and M >= 800000 and (forms & 4):
            # the out-stage (project) convs of the 112x112 / 56x56 stages: contiguous pixel range per workgroup (segment mode of
            # csrc/mnas_pwbwd.hip) and one resident round of workgroups instead of tiles strided over a 1024-wide grid:
            # 48 -> 16 at 112x112 200 -> 189 us, 72 -> 24 at 56x56 87 -> 83 us (same call); the expand forms (3-4 resident
            # workgroups per CU) and 240 -> 40 at 28x28 lose with it (16 -> 48: 155 -> 220 us at 512 segments)
            tile = lib.mnas_pw_bwd_tile_pixels(ci.cin, Co)
            nparts = max(1, min(nparts, eng.pw_bwd_segments))
            seg = _cdiv(_cdiv(M, nparts), tile) * tile
            nparts = _cdiv(M, seg)
        ops.add(L.OP_PW_BWD, M=M, Ci=ci.cin, Co=Co, nparts=nparts, gin_masked=masked, seg_px=seg, **fields)
        if eng.merge_post:
            self._queue_wgrad(ops, wsc, nparts, Co, ci.cin, 1, False, eng.gptr(ci, 0))
        else:
            ops.add(L.OP_WGRAD_FINALIZE, nsplit=nparts, Co=Co, Ci=ci.cin, taps=1, accumulate=1, partial=eng.scratch_wgrad2, grad=eng.gptr(ci, 0))
        return gin, (nparts if rt is not None else 0)

    def _bwd_gemm(self, ops, rec, gy, dyb, resid, need_gin, rt, WS):
        """weight gradient (k_wgrad, side stream if any) + input gradient as an implicit GEMM / transposed convolution.
        dyb: the materialised dy of a dense conv, or None (dy formed on load from gy)"""
        eng, lib, N, ci, Hi, Wi = self.eng, self.eng.lib, self.N, rec.ci, rec.Hi, rec.Wi
        Ho, Wo, Co, taps = rec.out.H, rec.out.W, ci.cout, ci.k * ci.k
        dy = gy if dyb is None else (dyb, None, None)
        # pixel splits: as many as keep slabs x splits within the workgroup budget (rounding UP put 513-540 workgroups on the
        # 512 resident slots of most launches: a second, nearly empty round)
        slabs = lib.mnas_conv_wgrad_slabs(Co, ci.cin, taps)
        nsp = max(1, min(eng.wgrad_wgs // slabs, _cdiv(N * Ho * Wo, 256)))
        # partial[nsp][Co][K] must fit the scratch _setup sized for 1024 workgroups (Engine.wgrad_wgs is public)
        nsp = max(1, min(nsp, eng.scratch_wgrad.numel() // (Co * ci.cin * taps)))
        ops.add(L.OP_CONV_WGRAD, WS, N=N, Hi=Hi, Wi=Wi, Ci=ci.cin, Ho=Ho, Wo=Wo, Co=Co, kh=ci.k, kw=ci.k, stride=ci.stride, pad=ci.pad,
                nsplit=nsp, x=rec.a_in, dy=dy, partial=eng.scratch_wgrad)
        ops.add(L.OP_WGRAD_FINALIZE, WS, nsplit=nsp, Co=Co, Ci=ci.cin, taps=taps, accumulate=1, partial=eng.scratch_wgrad, grad=eng.gptr(ci, 0))
        if not need_gin:
            return None, 0
        gin = self._new((N, Hi, Wi, ci.cin))
        nparts = self._igemm_parts(1, N * Hi * Wi, Co, ci.cin, taps, eng.igemm_dgrad_parts)
        plain_dense = ci.kind == "dense" and dyb is not None and resid is None
        tconv = eng.use_tconv and plain_dense and self._tconv_ok.get(id(ci), False) and Hi == 2 * Ho and Wi == 2 * Wo
        if tconv:
            tp = lib.mnas_tconv_parts(N, Ho, Wo, Co, ci.cin)       # (-1: a form that needs a larger batch)
            tconv = tp > 0
            nparts = tp if tconv else nparts
        if plain_dense and not tconv:
            ip = lib.mnas_conv_img_parts(1, N, Ho, Wo, Co, Hi, Wi, ci.cin, ci.k, ci.stride, ci.pad)
            nparts = ip if ip > 0 else nparts
        red = {} if rt is None else dict(stats=eng.scratch_red, red_y=rt[0], red_bn=rt[1])
        if tconv:
            # stride-2 3x3: transposed convolution over the materialised dy (csrc/mnas_tconv.hip)
            ops.add(L.OP_TCONV_DGRAD, N=N, Ho=Ho, Wo=Wo, Co=Co, Ci=ci.cin, nparts=nparts, dy=dyb, w=ci.w_tconv, out=gin, **red)
        else:
            ops.add(L.OP_CONV_GEMM, mode=1, N=N, Hi=Ho, Wi=Wo, Ci=Co, Ho=Hi, Wo=Wi, Co=ci.cin, kh=ci.k, kw=ci.k, stride=ci.stride,
                    pad=ci.pad, nparts=nparts, grad=dy, w=ci.w_dgrad, resid=resid, out=gin, **red)
        return gin, (nparts if rt is not None else 0)

    def _feeds_fused_dw(self, act: _Act):
        """True if the ConvBlock that produced the virtual activation `act` is a depthwise conv whose backward runs as the fused
        sweep (the only mnas_dw_bwd form that takes a masked gradient)."""
        for rec in self._records:
            if rec.out is act or (rec.out.data is act.data and rec.out.bn is act.bn):
                ci = rec.ci
                # ... and carries the fused reduce (its own input is a virtual activation), the form g_masked exists for
                return (ci.kind == "dw" and ci.stride == 1 and ci.k in self.eng.dw_fused_k and rec.a_in is not None and rec.a_in.bn is not None
                        and rec is not self._end_rec)
        return False

    def _conv_bwd_se_proj(self, ops: _OpList, rec, g, g_reduced, se_rec):
        """Backward of the project conv of a squeeze-excite block whose excitation is applied on load.  Returns (gs, du): the input
        gradient wrt the GATED activation and dL/du (fp32 [N][E])."""
        eng, N, ci, kseg = self.eng, self.N, rec.ci, se_rec.kseg
        Co, HW = ci.cout, rec.Hi * rec.Wi
        gy = self._bn_bwd(ops, rec, g, g_reduced)
        gs = self._new((N, rec.Hi, rec.Wi, ci.cin))
        du = self._new((N, ci.cin), torch.float32)
        wsc = self._next_scratch() if eng.merge_post else eng.scratch_wgrad2
        ops.add(L.OP_PW_BWD, M=N * HW, Ci=ci.cin, Co=Co, nparts=N * kseg, gin_masked=0, seg_px=HW // kseg,
                x=se_rec.h2, dy=gy, w=ci.w_dgrad, gin=gs, wpartial=wsc)
        ops.add(L.OP_SE_PROJ_FIN, N=N, kseg=kseg, Co=Co, Ci=ci.cin, accumulate=1,
                wpartial=wsc, u=se_rec.u, w=ci.mod.conv.weight, grad=eng.gptr(ci, 0), du=du)
        return gs, du

    def _se_bwd(self, ops: _OpList, se_rec, gs, du=None):
        """Backward of the squeeze-excite stage: gs = dL/d(a2 * s) from the project conv's input gradient -> dL/d a2, and the
        SE parameters' gradients (accumulated into the flat buffer; shared blocks sum their applications).  du: dL/du when the
        project conv's backward already produced it (excitation on load), else it is reduced here from (gs, a2)."""
        eng, lib, N = self.eng, self.eng.lib, self.N
        se, h2, z, hb, u = se_rec.se, se_rec.h2, se_rec.z, se_rec.hb, se_rec.u
        E_, R_ = se.channels, se.reduced
        HWl = h2.H * h2.W
        fc1, fc2 = se.mod.fc1, se.mod.fc2
        dh = self._new((N, R_), torch.float32)
        dzp = self._new((N, E_), torch.float32)
        ga = self._new((N, h2.H, h2.W, E_))
        if du is None:
            du = self._new((N, E_), torch.float32)
            sb = lib.mnas_se_scratch_bytes(N, HWl, E_)
            if sb < 0:
                raise RuntimeError("unsupported squeeze-excite shape %s" % ((N, HWl, E_),))
            dup = self._new((sb // 4,), torch.float32)
            ops.add(L.OP_SE_BWD_REDUCE, N=N, HW=HWl, C=E_, gs=gs, a=h2, u=u, du=du, scratch=dup)
        if eng.se_fused_mlp and lib.mnas_se_fc_supported(E_, R_):
            # the MLP backward in one op (two kernels: per-image dh / dz, then the parameter gradients; csrc/mnas_se.hip)
            ops.add(L.OP_SE_FC_BWD, N=N, E=E_, R=R_, accumulate=1, du=du, z=z, hb=hb, w1=fc1.weight, w2=fc2.weight, dh=dh, dz=dzp,
                    dw1=eng.gptr(se, 0), db1=eng.gptr(se, 1), dw2=eng.gptr(se, 2), db2=eng.gptr(se, 3))
        else:
            # Engine.se_fused_mlp = False (the A/B baseline): four mnas_head_linear_* launches
            # fc2: dW2 += du^T hb, db2 += sum du ; dh = (du W2) * [hb > 0]
            fc = dict(N=N, I=R_, O=E_, relu=0, x=hb, w=fc2.weight, dz=du)
            ops.add(L.OP_HEAD_LINEAR, accumulate=1, which=1, dw=eng.gptr(se, 2), db=eng.gptr(se, 3), **fc)
            ops.add(L.OP_HEAD_LINEAR, accumulate=0, which=2, dx=dh, relu_mask=hb, **fc)
            # fc1: dW1 += dh^T z, db1 += sum dh ; dz = dh W1
            fc = dict(N=N, I=E_, O=R_, relu=1, x=z, w=fc1.weight, dz=dh)
            ops.add(L.OP_HEAD_LINEAR, accumulate=1, which=1, dw=eng.gptr(se, 0), db=eng.gptr(se, 1), **fc)
            ops.add(L.OP_HEAD_LINEAR, accumulate=0, which=2, dx=dzp, **fc)
        # the BatchNorm2-backward reduce of the depthwise conv rides in the same pass (ga is its g; h2 = its raw output + bnbuf)
        ncols = lib.mnas_se_bwd_apply_cols(N, HWl, E_)
        fused = h2.bn is not None and 0 < ncols <= _STATS_PARTS
        red = dict(red_y=h2.data, red_bn=h2.bn, red_partial=eng.scratch_red) if fused else {}
        ops.add(L.OP_SE_BWD_APPLY, N=N, HW=HWl, C=E_, gs=gs, u=u, dz=dzp, out=ga, **red)
        return ga, (ncols if fused else 0)
