"""Execution engine: compiles (launch_plan.py) a subtree of the drop-in modules (mnasnet.py) into a static PROGRAM of HIP
kernel launches (include/mnas.h) per (batch, height, width, mode) and runs it with ONE host->library call
per forward / per backward segment (mnas_run_ops_multi: main stream + an OPTIONAL side stream for weight-gradient kernels,
Engine.use_side_stream).

Mirrors, for this path, what autograd + ATen do for the reference:
    forward   Mnasnet.features(x)                /root/reference/src/models/mnasnet.py:211-213
    backward  loss.backward() through it          /root/reference/src/train.py:439
but MI355X-first: NHWC bf16 activations resident in HBM (nothing is recomputed: 288 GB), BatchNorm+ReLU
fused into the consumers' loads, BatchNorm statistics fused into the producers' epilogues, all buffers
allocated once per shape, no Python per-layer dispatch on the step path.

Autograd contract: parameters are inputs of one autograd.Function, so loss.backward() reaches
us (tensor hooks registered on parameters -- register_hook / post-accumulate-grad hooks -- do NOT fire: the gradients
bypass AccumulateGrad; DDP-style hook-driven reducers must use train_step.Trainer's stage-done callback instead); weight/BN gradients are written by the kernels straight into a flat fp32 buffer whose slices ARE the
parameters' ``.grad`` (None -> attached, already ours -> accumulated, foreign tensor -> added into it), the
same observable behaviour as autograd's AccumulateGrad, without ~110 tiny copy kernels.  Shared blocks
accumulate their ``layers`` contributions; in train mode ``conv.bias.grad`` is exactly zero (batch-statistics
BatchNorm cancels the bias; the reference gets ~1e-5 rounding noise there).

Several forwards may be alive at once (up to _MAX_PROGRAMS_PER_SHAPE per shape and mode, any number of shapes and modes, no-grad
forwards in between): a Program owns its activations and BatchNorm coefficient blocks, so a backward depends only on its own
program, and any interleaving of forwards and backwards gives, bit for bit, the outputs, input gradients, running statistics (forward
order) and accumulated ``.grad`` (backward order) of the same jobs run one after the other (tests/test_gpu_lifetimes.py).
Stale state: what is NOT per program is read at backward time where it lives then -- the packed weights (re-packed by every forward),
``conv.bias`` / the stem's and squeeze-excite's weights (read in place) and, for the stem's weight gradient, the caller's batch.  The
rule is autograd's for saved tensors: between a forward and its backward no parameter of the subtree and (when the stem trains)
not the batch may be modified in place, and no parameter or BatchNorm buffer may get new storage.  The forward keeps their
``_version`` counters and the storage signature on its lease and the backward compares them (Engine.check_unchanged): a change
raises a RuntimeError that names it and asks for the forward again, instead of returning a finite gradient of nothing.  Replacing
storage (``p.data = ...``) while a forward is alive makes the NEXT forward raise too (reset_programs) until that output is dropped.
Not seen: writes that bypass the version counter (``p.data.mul_()``, kernels writing through raw pointers such as Trainer's fused
optimizers) -- do not run Trainer.step between a module-path forward and its backward.

Frozen BatchNorm statistics: a TRACKED forward of a subtree that is entirely in eval mode (``model.train();
model.features.eval()``, classifiers.FineTuneModelPool.freeze_bn) runs the frozen program (launch_plan.LaunchPlan,
frozen_bn): the eval forward, bit for bit, with its activations kept (the same launches without squeeze-excite; with
it, a block whose project conv has no gate-on-load backward at that size reads the materialised a*s where plain
inference gates on load -- the same values by another launch, LaunchPlan._se_onload_kseg), and a backward that gives
every parameter its gradient while the running buffers stay untouched.  There ``conv.bias.grad`` is NOT zero (s * sum dz).  A no-grad eval forward stays the
plain eval program; a subtree in mixed modes still raises.  The frozen program holds every backward buffer and a lease
until its output dies, so inference belongs under ``torch.no_grad()``: more than _MAX_PROGRAMS_PER_SHAPE tracked
eval-mode outputs alive at once raise.

Frozen stage prefix: the backward of a tracked forward ends at Engine.first_trainable_step(), the first step that owns a parameter
with ``requires_grad`` (classifiers.FineTuneModelPool.freeze(upto=k)); the steps in front of it get no backward launch and no
backward buffer (launch_plan.LaunchPlan, first_trainable).  The boundary is read at every forward and is part of the program key,
so changing ``requires_grad`` between two steps selects another program; ``x.requires_grad`` needs the whole backward.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib as L
from .launch_plan import LaunchPlan, _STATS_PARTS, _STEM_WGRAD_PARTS_MAX, _cdiv, se_segments_per_image  # noqa: F401  (re-exported)


class _ConvInfo:
    """One unique ConvBlock (shared blocks appear once)."""

    def __init__(self, mod, stage):
        conv, bn = mod.conv, mod.bn
        self.mod, self.stage = mod, stage
        self.cin, self.cout = conv.in_channels, conv.out_channels
        self.k = conv.kernel_size[0]
        self.stride, self.pad, self.groups = conv.stride[0], conv.padding[0], conv.groups
        if conv.kernel_size[0] != conv.kernel_size[1] or conv.stride[0] != conv.stride[1]:
            raise NotImplementedError("square kernels / strides only")
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError("BatchNorm2d(affine, track_running_stats, momentum=float) only")
        if self.groups == 1 and self.k == 1:
            if self.stride != 1 or self.pad != 0:
                raise NotImplementedError("1x1 convs are stride 1 / pad 0 in this network")
            self.kind = "pw"
        elif self.groups == self.cin == self.cout and self.groups > 1:
            if self.k not in (3, 5) or self.stride not in (1, 2) or self.pad != self.k // 2:
                raise NotImplementedError("depthwise: k in {3,5}, stride 1 or 2, pad k//2 (mnasnet.py:73-81,122-125)")
            self.kind = "dw"
        elif self.groups == 1 and self.k == 3 and self.pad == 1 and self.cin == 3 and self.stride == 2:
            self.kind = "stem"
        elif self.groups == 1 and self.k == 3 and self.pad == 1:
            self.kind = "dense"
        else:
            raise NotImplementedError("unsupported ConvBlock geometry")
        if self.kind != "stem" and (self.cin % 8 or self.cout % 8):
            raise NotImplementedError("channel counts must be multiples of 8")
        self.params = [conv.weight, conv.bias, bn.weight, bn.bias]
        self.gslice = {}            # name -> (offset, numel) in the flat grad buffer

    def out_hw(self, H, W):
        return ((H + 2 * self.pad - self.k) // self.stride + 1, (W + 2 * self.pad - self.k) // self.stride + 1)


class _SEInfo:
    """One unique SqueezeExcite module (build-defined SE variant): parameter bookkeeping like _ConvInfo."""

    def __init__(self, mod, stage):
        self.mod, self.stage = mod, stage
        self.channels, self.reduced = mod.fc1.in_features, mod.fc1.out_features
        self.params = [mod.fc1.weight, mod.fc1.bias, mod.fc2.weight, mod.fc2.bias]
        self.gslice = {}


def _trace(root, se_map=None):
    """Flatten a module subtree into steps: ("conv", ConvBlock, stage) / ("block", [e,d,p], stage).  se_map (optional dict)
    receives id(expand ConvBlock) -> SqueezeExcite module for blocks that carry one."""
    steps = []

    def rec(m, stage):
        name = type(m).__name__
        if name == "ConvBlock":
            steps.append(("conv", m, stage))
        elif name == "MBConv_block":
            steps.append(("block", list(m.sequence), stage))
            if se_map is not None and getattr(m, "se", None) is not None:
                se_map[id(m.sequence[0])] = m.se
        elif name in ("SepConv", "MBConv"):
            for c in m.sequence:
                rec(c, stage)
        elif name == "Mnasnet":
            rec(m.features, stage)
        elif isinstance(m, nn.Sequential):
            for i, c in enumerate(m):
                rec(c, i if stage is None else stage)
        else:
            raise TypeError("cannot compile %s for the HIP engine" % name)

    rec(root, None)
    return [(op, m, 0 if st is None else st) for op, m, st in steps]


class Program(LaunchPlan):
    """launch_plan.LaunchPlan (all buffers + launch lists of one (N, H, W, training, need_dx) configuration) and its run-time half:
    the run-time pointers are patched into the lists, which are launched per op or replayed as hipGraphs."""

    def __init__(self, eng: "Engine", N, H, W, training, need_dx, pooled=False, in_u8=False, *, frozen_bn=False, first_trainable=0):
        self._graphs = {}
        self.busy = False
        self._out_buf = self._gout_buf = self._x_buf = self._x_direct = None
        super().__init__(eng, N, H, W, training, need_dx, pooled, in_u8, frozen_bn=frozen_bn, first_trainable=first_trainable)

    # ------------------------------------------------------------------------------------------
    def _run(self, arr, n, what):
        failed = C.c_int(-1)
        streams = (C.c_void_p * 2)(L.cur_stream(), self.eng.side_stream_handle())
        live_events = self._built_prof and self.eng.profile_gate.value != 0      # bracketing event records: per-launch path
        # (not with the second stream: a segment may fork onto it and join only at the end of a later segment -- an unjoined capture)
        if self.eng.use_graphs and n > 1 and not live_events and not self._built_side:
            # the list as a hipGraph (csrc/mnas_abi.hip mnas_graph_create): captured at first use and whenever a run-time
            # pointer of the list (input batch, output, incoming gradient) or the event-record gate has changed since
            key = hash(bytes(arr))
            slot = self._graphs.setdefault(id(arr), {"exec": None, "key": None, "miss": 0})
            if slot["key"] != key and slot["miss"] < 4:
                if slot["exec"] is not None:
                    # the previous launch of this exec may still be running (the host enqueues a step in < 1 ms of a 10 ms step)
                    # and the exec owns its kernel arguments: wait for the device first (at most 4 re-captures per list)
                    torch.cuda.synchronize(self.eng.device)
                    self.eng.lib.mnas_graph_destroy(slot["exec"])
                    slot["exec"] = None
                    slot["miss"] += 1             # a list whose pointers change every step is not worth capturing: fall through
                ex = C.c_void_p()
                # capture on a stream of our own (the legacy default stream cannot capture); the graph is LAUNCHED on the current one
                if self.eng._capture_stream is None or self.eng._capture_stream.device != self.eng.device:
                    self.eng._capture_stream = torch.cuda.Stream(device=self.eng.device)
                cap = (C.c_void_p * 2)(self.eng._capture_stream.cuda_stream, streams[1])
                rc = self.eng.lib.mnas_graph_create(arr, n, cap, 2, C.byref(ex), C.byref(failed))
                if rc != 0:
                    raise RuntimeError("%s: graph capture failed with code %d at op %d" % (what, rc, failed.value))
                slot["exec"], slot["key"] = ex, key
            if slot["key"] == key and slot["exec"] is not None:
                rc = self.eng.lib.mnas_graph_launch(slot["exec"], streams[0])
                if rc != 0:
                    raise RuntimeError("%s: hipGraphLaunch failed with code %d" % (what, rc))
                return
        rc = self.eng.lib.mnas_run_ops_multi(arr, n, streams, 2, C.byref(failed))
        if rc != 0:
            raise RuntimeError("%s: mnas_run_ops failed with code %d at op %d (opcode %d)" %
                               (what, rc, failed.value, arr[failed.value].opcode if failed.value >= 0 else -1))

    def destroy_graphs(self):
        """Destroy the captured graph executables -- after a device sync: one of them may still be executing."""
        slots = [s for s in self._graphs.values() if s["exec"] is not None]
        if not slots:
            return
        torch.cuda.synchronize(self.eng.device)
        for slot in slots:
            self.eng.lib.mnas_graph_destroy(slot["exec"])
            slot["exec"] = None

    def __del__(self):
        try:
            self.destroy_graphs()
        except Exception:
            pass

    def run_forward(self, x, static_io=False):
        """static_io (Trainer's autograd-free path with Engine.use_graphs): the output lives in a buffer of the program, so that the
        captured graph's pointers stay valid from step to step (the caller consumes it before the next forward of this program)."""
        if static_io and self.eng.use_graphs:
            if self._out_buf is None or self._out_buf.device != x.device:
                self._out_buf = torch.empty(self.out_shape, dtype=torch.float32, device=x.device)
            out = self._out_buf
            # the input: a batch that is the same tensor step after step (a resident benchmark batch) is read in place; as soon as
            # a different tensor arrives (a data loader), every batch is copied into a buffer of the program first (fp32 bs 256:
            # 154 MB, ~35 us; uint8: a quarter) so that the captured graphs stay valid
            if self._x_direct is None:
                self._x_direct = x.data_ptr()
            if self._x_buf is not None or x.data_ptr() != self._x_direct:
                if self._x_buf is None or self._x_buf.shape != x.shape or self._x_buf.dtype != x.dtype or self._x_buf.device != x.device:
                    self._x_buf = torch.empty_like(x)
                self._x_buf.copy_(x)
                x = self._x_buf
        else:
            out = torch.empty(self.out_shape, dtype=torch.float32, device=x.device)
        for j, slot in self.patch_x:
            self.fwd_ops[j].p[slot] = x.data_ptr()
        j, slot = self.patch_out
        self.fwd_ops[j].p[slot] = out.data_ptr()
        self.x_ref = x
        self._run(self.fwd_ops, self.fwd_n, "forward")
        return out

    def run_backward(self, gout, on_stage_done: Optional[Callable[[int], None]] = None, static_io=False):
        if not self.bwd_segments:
            raise RuntimeError("this program has no backward: it was built for inference or with every step frozen")
        if static_io and self.eng.use_graphs:
            if self._gout_buf is None or self._gout_buf.shape != gout.shape or self._gout_buf.device != gout.device:
                self._gout_buf = torch.empty_like(gout)
            self._gout_buf.copy_(gout)                       # (a few hundred KB) keeps the captured pointer valid
            gout = self._gout_buf
        segs = {st: (arr, n) for st, arr, n in self.bwd_segments}

        def patch(where, ptr):
            st, j, slot = where
            segs[st][0][j].p[slot] = ptr
            self.bwd_all[self._seg_off[st] + j].p[slot] = ptr

        patch(self.patch_gout, gout.data_ptr())
        if self.patch_x_bwd is not None:
            patch(self.patch_x_bwd, self.x_ref.data_ptr())
        dx = None
        if self.patch_dx is not None:
            dx = torch.empty((self.N, self.in_channels, self.H, self.W), dtype=torch.float32, device=gout.device)
            patch(self.patch_dx, dx.data_ptr())
        if self.eng.use_graphs and on_stage_done is None and not self._built_side:
            self._run(self.bwd_all, self.bwd_all_n, "backward")
            self.x_ref = None
            return dx
        for st, arr, n in self.bwd_segments:
            self._run(arr, n, "backward[stage %d]" % st)
            if on_stage_done is not None:
                on_stage_done(st)
        self.x_ref = None
        return dx

_MAX_PROGRAMS_PER_SHAPE = 4     # forwards kept alive simultaneously per (N,H,W,mode): beyond this the caller is leaking graphs


class _Lease:
    """Ties a Program's activation buffers to the autograd graph of ONE forward.  The program is handed back when
    backward has consumed it OR when the graph is dropped without a backward (exception between forward and backward,
    LR finder, BatchNorm recalibration pass, ...): ``ctx`` dies with the graph and takes this object with it."""
    __slots__ = ("prog", "consumed", "sig", "versions", "x_version", "__weakref__")

    def __init__(self, prog, sig=None, versions=(), x_version=None):
        self.prog, self.consumed = prog, False
        # forward-time facts, compared in backward (Engine.check_unchanged): the storage signature, every parameter's version counter
        # and, where the backward reads the batch, the batch's
        self.sig, self.versions, self.x_version = sig, versions, x_version
        prog.busy = True

    def release(self):
        if self.prog is not None:
            self.prog.busy = False
            self.prog = None

    def __del__(self):
        self.release()


class _EngineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, track, pooled, x, *params):
        need_dx = track and x.requires_grad
        training = eng.root.training
        # a tracked forward in eval mode trains on the running statistics (frozen program); without tracking it is plain inference
        frozen = track and not training
        # the backward ends at the first step that owns a trainable parameter; an input gradient needs all of it
        first = 0 if (need_dx or not track) else eng.first_trainable_step()
        prog = eng.program(x.shape[0], x.shape[2], x.shape[3], training or frozen, need_dx, pooled, x.dtype == torch.uint8,
                           frozen_bn=frozen, first_trainable=first)
        out = prog.run_forward(x)
        ctx.eng = eng
        ctx.lease = None
        if track:
            ctx.lease = _Lease(prog, eng._sig, tuple(p._version for p in eng.params),
                               prog.x_ref._version if prog.patch_x_bwd is not None else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        lease, eng = ctx.lease, ctx.eng
        if lease is None:
            raise RuntimeError("backward through a no-grad engine forward")
        if lease.consumed or lease.prog is None:
            # the activation buffers belong to a per-shape program that later forwards reuse: a second backward
            # (retain_graph=True) would read overwritten activations
            raise RuntimeError("the HIP engine keeps activations for ONE backward per forward; run the forward again "
                               "(retain_graph=True is not supported through mnasnet_pytorch_amd modules)")
        prog = lease.prog
        try:
            eng.check_unchanged(lease)
            accumulate = eng.prepare_grads()
            dx = prog.run_backward(gout.contiguous().float(), eng.on_stage_done)
            eng.finish_grads(accumulate)
        finally:
            lease.consumed = True
            lease.release()
        return (None, None, None, dx) + (None,) * len(eng.params)


class Engine:
    """Owns the packed weights, scratch space, flat gradient buffer and per-shape programs of one module
    subtree."""

    def __init__(self, root: nn.Module):
        self.root = root
        self._se_mods = {}
        self.steps = _trace(root, self._se_mods)
        self.lib = None
        self.device = None
        self.programs: Dict[tuple, List[Program]] = {}
        self.on_stage_done: Optional[Callable[[int], None]] = None
        # unique ConvBlocks in first-use order
        self.info: Dict[int, _ConvInfo] = {}
        self.convs: List[_ConvInfo] = []
        for op, m, stage in self.steps:
            for cb in ([m] if op == "conv" else m):
                if id(cb) not in self.info:
                    ci = _ConvInfo(cb, stage)
                    self.info[id(cb)] = ci
                    self.convs.append(ci)
        for n, (op, m, stage) in enumerate(self.steps):
            for cb in ([m] if op == "conv" else m):
                if self.info[id(cb)].kind == "stem" and n != 0:
                    raise NotImplementedError("a 3-channel stride-2 conv is only supported as the first layer")
        # squeeze-excite modules (SE variant only): one _SEInfo per unique module, keyed by its block's expand ConvBlock
        self.se_info: Dict[int, _SEInfo] = {}
        self.ses: List[_SEInfo] = []
        by_mod = {}
        for op, m, stage in self.steps:
            if op == "block" and id(m[0]) in self._se_mods:
                se = self._se_mods[id(m[0])]
                if id(se) not in by_mod:
                    by_mod[id(se)] = _SEInfo(se, stage)
                    self.ses.append(by_mod[id(se)])
                self.se_info[id(m[0])] = by_mod[id(se)]
        self.param_owners = self.convs + self.ses      # everything that owns parameters, in the flat-gradient order below
        # flat gradient layout: later stages first (their gradients are complete first in backward)
        self.params: List[nn.Parameter] = []
        off = 0
        self.stage_ranges: Dict[int, List[int]] = {}
        for ci in sorted(self.param_owners, key=lambda c: -c.stage):
            a = off
            for j, p in enumerate(ci.params):
                ci.gslice[j] = (off, p.numel())
                off += p.numel()
                self.params.append(p)
            r = self.stage_ranges.setdefault(ci.stage, [a, off])
            r[0], r[1] = min(r[0], a), max(r[1], off)
        self.grad_numel = off
        self._sig = None
        self._ext_grad: Optional[torch.Tensor] = None
        # weight-gradient kernels on a second HIP stream, concurrent with the input-gradient chain.  +14 % when introduced (round 1);
        # by round 3 the main-stream kernels and k_wgrad_t fill the chip on their own and the overlap only trades time between the
        # two streams (11.17-11.21 ms with it, 11.07-11.13 without, same call) -- and it hid per-kernel gains on the main stream
        # (the K-streaming input gradient: neutral with the side stream, -0.1 ms without).  Off by default; the path stays tested.
        self.use_graphs = False          # launch lists replayed as hipGraphs (Program._run)
        self._capture_stream = None
        self.use_side_stream = False
        self.side_stream_max_pixels = 1 << 40     # with use_side_stream: only layers with at most this many output pixels fork
        # workgroups of a k_wgrad launch (pixel splits x 64x64 slabs): 512 rather than 1024 leaves the main stream's persistent
        # grids more of the chip while it runs beside them (11.57 vs 11.66 ms/step, three same-call A/B pairs; 256: 11.77)
        self.wgrad_wgs = 512
        self.join_stages = None          # stages after which the main stream joins the side stream (None: see Program)
        self.use_tconv = True            # stride-2 dense 3x3 input gradient as a transposed convolution (csrc/mnas_tconv.hip)
        self.merge_post = True           # BatchNorm-backward finalize + weight-gradient reductions of the main stream in one launch
        self.materialize_dy = True       # dense 3x3 convs: dy formed once (mnas_dy_materialize), gathered plain by dgrad / wgrad
        # depthwise kernel sizes whose backward runs as ONE fused sweep (input gradient + weight gradient + reduce).  5x5 too:
        # with 2-row DMA groups the fused form gets full-width strips and beats the two launches (155 vs 210 us at 56x56)
        # although it needs all 256 VGPRs; (3,) selects the split form (input gradient on main, weight gradient on side)
        self.dw_fused_k = (3, 5)
        # 1x1 convs with at least this many pixels use the fused backward (mnas_pw_bwd) when the shape is supported: measured
        # per launch at bs 256 against the dgrad + wgrad pair: 201 vs 399 us (16->48 @112^2), 233 vs 331 (48->16), 119 vs 285
        # (32->16), 90 vs 199 (24->72 @56^2), 105 vs 195 (72->24), 81 vs 141 (40->240 @28^2), 111 vs 175 (240->40)
        self.pw_fused_min_pixels = 50000
        # narrowing (project) 1x1 convs below this pixel count: DMA-pipelined input gradient on the main stream
        # (csrc/mnas_pwf.hip MODE 1) + weight gradient on the side stream, instead of the fused sweep.  Off: alone the input
        # gradient takes 68 us against the fused kernel's 116 (576->96 at 14x14, bs 256), but next to the side stream's
        # k_wgrad it takes 130 us and the step is 0.1 ms slower (12.56 vs 12.44 ms)
        self.pw_split_max_pixels = 0
        # expand convs of the 112x112 / 56x56 stages (16->48, 24->72): the fused 1x1 backward recomputes the conv's raw output
        # from its (narrow) input instead of reading the t-times wider stored tensor (mnas_pw_bwd RECOMP; round 4:
        # 209 -> 155 us per launch at 112x112, bit-identical results)
        self.pw_recompute_y = True
        # project convs' fused backward (out-stage forms) store the depthwise conv's incoming gradient already masked with its ReLU
        # (dz = g*[s*y+t>0], the mask the fused reduce computes anyway); the depthwise sweep's dy-on-read then skips the mask:
        # 40 of the 5x5 row body's ~530 vector instructions (round 4; results bit-identical)
        self.dw_masked_g = True
        self.se_on_load = True           # squeeze-excite excitation applied in the project conv's load (forward) / folded into its
                                         # weight-gradient slabs (backward) where the kernels support the shape; False: k_se_scale
        self.se_fused_mlp = True         # the squeeze-excite MLP as mnas_se_fc_fwd / mnas_se_fc_bwd (1 + 2 kernels per block instead of 3 + 4)
        self.pw_bwd_segments = 512       # > 0: the project convs' fused backward at >= 800 k pixels walks contiguous pixel segments,
                                         # at most this many workgroups (0: tiles strided over the grid everywhere)
        self.igemm_fwd_parts = 1024      # upper bound on the persistent pixel-workgroups of a k_igemm forward / input-gradient launch
        self.igemm_dgrad_parts = 1024
        self.dw_bwd_parts = 2048         # upper bound on the persistent workgroups of a depthwise backward launch (round 6: 1024 made
                                         # the 1280-item launches of the 14x14 / 7x7 stages walk 1.25 items per workgroup on 1020
                                         # workgroups; one item per workgroup: step 10.15 vs 10.19 ms, three interleaved pairs)
        self.pw_bwd_parts_large = 1024   # ... on the 112x112 / 56x56 stages
        self.pw_bwd_parts_mid = 512      # ... on the 28x28 stage
        self.pw_bwd_parts_small = 80     # persistent pixel-workgroups of the fused 1x1 backward on the 14x14 stage (x 6 channel slices): a
                                         # multiple of 8 (the slices of one pixel column share an XCD's L2) with 6 x 80 <= the 512 resident
                                         # slots; 85 -> 80: class -0.06 ms, 88 (528 workgroups, a second round): +0.15 ms
        self.side_stream = None
        self._in_norm, self._in_aff = None, {}
        self.profile_opcodes = None      # set of opcodes to bracket with HIP events (bench.py roofline leg)
        self.profile_filter = None       # optional predicate (opcode, ints) -> bool narrowing the bracketed launches
        self.profile_events = []         # [(tag, start_handle, stop_handle)]
        self.profile_gate = C.c_int(1)   # 0: the bracketing event records of the compiled programs are skipped (read at run time by
                                         # mnas_run_ops: bench.py switches them on for the last step of a timed window only)
        self._events = []                # every HIP event handle the compiled programs own (destroyed with them)
        self.first_conv = self.convs[0]      # (unique ConvBlocks are in first-use order)
        self.in_channels_hint = self.first_conv.cin
        self.starts_with_stem = self.first_conv.kind == "stem"

    # ---- device state ---------------------------------------------------------------------------
    def _signature(self):
        sig = [p.data_ptr() for p in self.params]
        for ci in self.convs:
            bn = ci.mod.bn
            sig += [bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr()]
        return tuple(sig)

    def _setup(self, device):
        self.lib = L.load()
        if self.device is not None:
            self.reset_programs()
        self.device = device
        self._validate_modules()
        if self.side_stream is not None and self.side_stream.device != device:
            self.side_stream = None          # re-created lazily on the new device (side_stream_handle)
        nbytes = self.lib.mnas_packed_bytes
        smax, wmax = 0, 0
        for ci in self.convs:
            if ci.kind in ("pw", "dense"):
                ci.w_fwd = torch.empty(nbytes(L.PACK_FWD, ci.cout, ci.cin, ci.k, ci.k), dtype=torch.uint8, device=device)
                ci.w_dgrad = torch.empty(nbytes(L.PACK_DGRAD, ci.cout, ci.cin, ci.k, ci.k), dtype=torch.uint8, device=device)
                ci.w_tconv = None
                # transposed-conv form of the stride-2 input gradient: the buffer exists for every stride-2 dense conv (< 1 MB each);
                # whether a PROGRAM packs and uses it is decided from that program's real dy plane (Program.__init__)
                if ci.kind == "dense" and ci.stride == 2 and self.use_tconv and self.materialize_dy:
                    ci.w_tconv = torch.empty(nbytes(L.PACK_TCONV, ci.cout, ci.cin, 3, 3), dtype=torch.uint8, device=device)
                K = ci.k * ci.k * ci.cin
                slabs = self.lib.mnas_conv_wgrad_slabs(ci.cout, ci.cin, ci.k * ci.k)
                wmax = max(wmax, max(1, _cdiv(1024, slabs)) * ci.cout * K)
                if ci.kind == "pw" and self.lib.mnas_pw_bwd_supported(ci.cin, ci.cout):
                    wmax = max(wmax, 1024 * ci.cout * ci.cin)      # one slab per workgroup of the fused 1x1 backward
                if ci.kind == "pw":
                    wmax = max(wmax, 64 * ci.cout * ci.cin)        # fused block backward: one slab per image group (<= 64)
            elif ci.kind == "dw":
                ci.w_fwd = torch.empty(nbytes(L.PACK_DW, ci.cout, 1, ci.k, ci.k), dtype=torch.uint8, device=device)
                wmax = max(wmax, max(1024, self.dw_bwd_parts) * ci.k * ci.k * ci.cout)      # wpartial[rows <= nparts][k*k][C]
            else:
                ci.w_fwd = torch.empty(nbytes(L.PACK_FWD, ci.cout, 27, 1, 1), dtype=torch.uint8, device=device)
                wmax = max(wmax, _STEM_WGRAD_PARTS_MAX * ci.cout * 27)   # k_stem_wgrad writes partial[nparts][Co][27]
            smax = max(smax, ci.cout)
        self.scratch_stats = torch.empty(_STATS_PARTS * 2 * smax, dtype=torch.float32, device=device)
        self.scratch_wgrad = torch.empty(wmax, dtype=torch.float32, device=device)
        self.scratch_wgrad2 = torch.empty(wmax, dtype=torch.float32, device=device)
        self.scratch_wgrad3 = torch.empty(wmax, dtype=torch.float32, device=device)      # main-stream producers rotate over 2..4:
        self.scratch_wgrad4 = torch.empty(wmax, dtype=torch.float32, device=device)      # a table is reduced up to two launches later
        self.scratch_red = torch.empty(_STATS_PARTS * 2 * smax, dtype=torch.float32, device=device)   # fused BN-bwd partials
        if self._ext_grad is not None:
            self.flat_grad = self._ext_grad
        else:
            self.flat_grad = torch.zeros(self.grad_numel, dtype=torch.float32, device=device)
        self.grad_views = []
        for ci in sorted(self.param_owners, key=lambda c: -c.stage):
            for j, p in enumerate(ci.params):
                o, n = ci.gslice[j]
                self.grad_views.append(self.flat_grad[o:o + n].view(p.shape))

    def _validate_modules(self):
        """The kernels read every parameter / buffer as dense fp32: anything else (model.half(), .bfloat16(),
        .double(), a non-contiguous view) must fail loudly instead of producing garbage."""
        for ci in self.convs:
            conv, bn = ci.mod.conv, ci.mod.bn
            named = [("conv.weight", conv.weight), ("conv.bias", conv.bias), ("bn.weight", bn.weight), ("bn.bias", bn.bias),
                     ("bn.running_mean", bn.running_mean), ("bn.running_var", bn.running_var)]
            for name, t in named:
                if t is None:
                    raise NotImplementedError("ConvBlock without %s" % name)
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise TypeError("mnasnet_pytorch_amd: %s must be contiguous float32 (got %s%s); the HIP path keeps fp32 "
                                    "master weights / statistics and bf16 activations internally -- do not call .half() / "
                                    ".bfloat16() / .double() on the model" %
                                    (name, t.dtype, "" if t.is_contiguous() else ", non-contiguous"))
            if bn.num_batches_tracked is not None and bn.num_batches_tracked.dtype != torch.int64:
                raise TypeError("bn.num_batches_tracked must be int64")
        for se in self.ses:
            for t in se.params:
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise TypeError("mnasnet_pytorch_amd: SqueezeExcite parameters must be contiguous float32")

    def _check_modes(self):
        """One mode per call: the launch list is compiled for root.training.  A submodule in a different mode (``bn.eval()`` under a
        training root) is not silently ignored; frozen-BN fine-tuning puts the WHOLE subtree in eval mode (module docstring)."""
        mode = self.root.training
        for m in self.root.modules():
            if m.training != mode:
                raise NotImplementedError(
                    "mixed train/eval modes inside one engine subtree (%s.training=%s, root.training=%s): per-submodule "
                    "BatchNorm freezing is not supported by the HIP engine" % (type(m).__name__, m.training, mode))

    def bind_grad_buffer(self, buf: Optional[torch.Tensor]):
        """Make the kernels write gradients into ``buf`` (fp32, ``grad_numel`` elements, engine layout: later
        stages first) instead of an engine-owned buffer -- used by train_step.Trainer so that ONE flat buffer
        feeds the RCCL all-reduce buckets and the fused Adam."""
        if buf is not None and (buf.numel() != self.grad_numel or buf.dtype != torch.float32 or not buf.is_contiguous()):
            raise ValueError("grad buffer must be contiguous fp32 with %d elements" % self.grad_numel)
        self._ext_grad = buf
        self._sig = None           # forces _setup (programs hold gradient pointers)

    def ensure_setup(self, device):
        sig = self._signature()
        if self.lib is None or self.device != device or sig != self._sig:
            self._setup(device)
            self._sig = sig

    def reset_programs(self):
        """Drop the compiled launch lists (they embed the profiling brackets); rebuilt lazily on the next call.
        The HIP events they own are destroyed (after a device sync: a launch list may still be in flight)."""
        if any(p.busy for lst in self.programs.values() for p in lst):
            raise RuntimeError("reset_programs() while a forward is waiting for its backward")
        for lst in self.programs.values():
            for p in lst:
                p.destroy_graphs()            # syncs first when a program holds a graph executable
        self.programs.clear()
        self.profile_events = []
        if self._events:
            torch.cuda.synchronize(self.device)
            for h in self._events:
                self.lib.mnas_event_destroy(h)
            self._events = []

    def side_stream_handle(self):
        """hipStream_t for stream slot 1 of mnas_run_ops_multi.  The second stream exists only when use_side_stream asks for it
        (created on first use); otherwise slot 1 is the current stream too and launch lists carry no stream-1 ops."""
        if not self.use_side_stream:
            return L.cur_stream()
        if self.side_stream is None:
            self.side_stream = torch.cuda.Stream(device=self.device)
        return self.side_stream.cuda_stream

    def new_event(self):
        h = C.c_void_p()
        L.check(self.lib.mnas_event_create(C.byref(h)), "event_create")
        self._events.append(h.value)
        return h.value

    def __del__(self):
        try:
            for h in self._events:
                self.lib.mnas_event_destroy(h)
        except Exception:       # interpreter shutdown
            pass

    def read_profile(self):
        """[(tag, ms)] for every bracketed op launch since the programs were built (call after a sync)."""
        out = []
        for tag, e0, e1 in self.profile_events:
            ms = C.c_float()
            if self.lib.mnas_event_elapsed_ms(e0, e1, C.byref(ms)) == 0:
                out.append((tag, ms.value))
        return out

    def gptr(self, ci: _ConvInfo, j: int):
        return self.flat_grad.data_ptr() + 4 * ci.gslice[j][0]

    def set_input_normalization(self, mean=None, std=None):
        """Fuse the dataset's ``transforms.Normalize(mean, std)`` (datasets.py:474-516 with the constants of classifiers.py:91-92)
        into the stem conv's input load: float images are read as (x - mean) / std, uint8 images as (x / 255 - mean) / std
        (a quarter of the PCIe / HBM bytes of the fp32 batch train.py:427 uploads).  None, None removes the transform."""
        if not self.starts_with_stem:
            raise RuntimeError("input normalisation is fused into the stem conv: this engine does not start with one")
        if mean is None or std is None:
            self._in_norm = None
        else:
            m = torch.as_tensor(mean, dtype=torch.float64).flatten()
            s = torch.as_tensor(std, dtype=torch.float64).flatten()
            if m.numel() != 3 or s.numel() != 3 or bool((s <= 0).any()):
                raise ValueError("mean / std must have 3 entries, std > 0")
            self._in_norm = (m, s)
        self._in_aff = {}
        if self.programs:
            self.reset_programs()

    def input_affine(self, u8: bool):
        """device float[2][3] (scale, shift) of the stem's fused input transform for float / uint8 images, or None"""
        if self._in_norm is None:
            return None
        t = self._in_aff.get((u8, self.device))
        if t is None:
            m, s = self._in_norm
            k = 255.0 if u8 else 1.0
            t = torch.stack([1.0 / (k * s), -m / s]).to(torch.float32).to(self.device).contiguous()
            self._in_aff[(u8, self.device)] = t
        return t

    def step_params(self, i: int) -> List[nn.Parameter]:
        """The parameters step ``i`` owns: its ConvBlocks' conv.weight, conv.bias, bn.weight, bn.bias and, for a block with
        squeeze-excite, the se.fc* parameters."""
        op, m, _ = self.steps[i]
        owners = [self.info[id(cb)] for cb in ([m] if op == "conv" else m)]
        if op == "block" and id(m[0]) in self.se_info:
            owners.append(self.se_info[id(m[0])])
        return [p for o in owners for p in o.params]

    def first_trainable_step(self) -> int:
        """The smallest index i such that step i owns a parameter with requires_grad, len(self.steps) if there is none: where the
        backward may end (LaunchPlan first_trainable).  Read from the modules at every call: freeze() / unfreeze() or a manual
        ``p.requires_grad = ...`` between two forwards selects another program.  The applications of a list-multiplied block share
        one module and flip together."""
        for i in range(len(self.steps)):
            if any(p.requires_grad for p in self.step_params(i)):
                return i
        return len(self.steps)

    def step_stage(self, i: int) -> int:
        """features.<stage> of step i; one past the last stage for i == len(self.steps)"""
        return self.steps[i][2] if i < len(self.steps) else self.steps[-1][2] + 1

    def program(self, N, H, W, training, need_dx, pooled=False, in_u8=False, *, frozen_bn=False, first_trainable=0) -> Program:
        key = (N, H, W, training, need_dx, pooled, bool(in_u8), bool(frozen_bn), int(first_trainable))
        lst = self.programs.setdefault(key, [])
        for p in lst:
            if not p.busy:
                return p
        if len(lst) >= _MAX_PROGRAMS_PER_SHAPE:
            raise RuntimeError(
                "%d forwards of shape %s are alive at once (their autograd graphs are still referenced and no backward "
                "has run): each holds a full set of activation buffers.  Drop the old outputs / call backward, or run "
                "under torch.no_grad()." % (len(lst), (N, self.in_channels_hint, H, W)))
        p = Program(self, N, H, W, training, need_dx, pooled, in_u8, frozen_bn=frozen_bn, first_trainable=first_trainable)
        lst.append(p)
        return p

    # ---- forward-time state a backward depends on ---------------------------------------------------
    def _param_name(self, p):
        for name, q in self.root.named_parameters():
            if q is p:
                return name
        return "<parameter of shape %s>" % (tuple(p.shape),)

    def check_unchanged(self, lease: _Lease):
        """A backward reads the packed weights, some parameters and (stem weight gradient) the batch where they live NOW, against
        activations of the forward: it is only the gradient of that forward if none of them changed since.  Raises otherwise
        (module docstring, "Stale state"); host-side only, nothing is launched."""
        if lease.sig is not None and self._signature() != lease.sig:
            raise RuntimeError("a parameter or BatchNorm buffer was given new storage (p.data = ..., .to(), ...) after the forward this "
                               "backward belongs to: its launch lists still name the old storage; run the forward again")
        for p, v in zip(self.params, lease.versions):
            if p._version != v:
                raise RuntimeError("parameter %s was modified in place between a forward and its backward (optimizer step, "
                                   "weight swap, mul_ ...): the backward would read the new weights against the old "
                                   "activations; run the forward again" % self._param_name(p))
        if lease.x_version is not None and lease.prog.x_ref is not None and lease.prog.x_ref._version != lease.x_version:
            raise RuntimeError("the input batch was modified in place between a forward and its backward: the stem's weight "
                               "gradient reads the batch in backward; run the forward again (or pass a copy)")

    # ---- .grad bookkeeping (AccumulateGrad semantics on a flat buffer) -----------------------------
    def prepare_grads(self):
        """Returns True if every live .grad is already one of our views (accumulate in place)."""
        ours, other = 0, 0
        for p, v in zip(self.params, self.grad_views):
            if not p.requires_grad:
                continue
            if p.grad is not None and p.grad.data_ptr() == v.data_ptr() and p.grad.shape == v.shape:
                ours += 1
            else:
                other += 1
        if ours and other:       # mixed: zero the slices that are not live accumulators, then accumulate
            for p, v in zip(self.params, self.grad_views):
                if not (p.grad is not None and p.grad.data_ptr() == v.data_ptr()):
                    v.zero_()
            return True
        if ours:
            return True
        self.flat_grad.zero_()
        return False

    def finish_grads(self, accumulate):
        for p, v in zip(self.params, self.grad_views):
            if not p.requires_grad:
                continue
            if p.grad is None:
                p.grad = v
            elif p.grad.data_ptr() != v.data_ptr():
                p.grad.add_(v)          # a foreign .grad tensor: add into it, like AccumulateGrad

    # ---- entry point ------------------------------------------------------------------------------
    def check_input(self, x: torch.Tensor):
        """Everything a launch list assumes about its input pointer; shared by forward() and Trainer.step's autograd-free path
        (a host or wrong-device pointer handed to the kernels is a GPU memory fault, not an exception)."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("mnasnet_pytorch_amd runs on MI355X only: got a %s tensor; there is no CPU/eager "
                               "fallback (use oracle/ in tests for a CPU reference)" % (x.device if isinstance(x, torch.Tensor) else type(x)))
        if x.dim() != 4:
            raise ValueError("expected NCHW input")
        if x.shape[1] != (3 if self.starts_with_stem else self.in_channels_hint):
            raise ValueError("expected %d input channels, got %d" % (3 if self.starts_with_stem else self.in_channels_hint, x.shape[1]))
        if x.shape[0] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
            raise ValueError("empty input %s" % (tuple(x.shape),))
        if any(p.device != x.device for p in self.params):
            raise RuntimeError("module parameters and input are on different devices")

    def forward(self, x: torch.Tensor, pooled: bool = False) -> torch.Tensor:
        """pooled=True returns the global average of the features, [N, C] fp32 (AdaptiveAvgPool2d(1) + flatten fused in)."""
        self.check_input(x)
        track = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.params))
        if x.dtype == torch.uint8 and self.starts_with_stem and self._in_norm is not None:
            x = x.contiguous()              # uint8 images stay uint8: the stem converts and normalises on load
        else:
            x = x.float().contiguous()      # train.py:427 input.float()
        self.ensure_setup(x.device)
        self._check_modes()
        return _EngineFn.apply(self, track, bool(pooled), x, *self.params)
