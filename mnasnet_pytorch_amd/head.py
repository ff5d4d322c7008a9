"""Native classifier head + loss: ``FineTuneModelPool.classifier`` (classifiers.py:56-89, an ``nn.Sequential`` of
Dropout / Linear / ReLU) and ``nn.CrossEntropyLoss`` (train.py:277) on the HIP library (csrc/mnas_head.hip).

Two entry points share the same kernels:

* :class:`NativeHead` ``.apply(x)`` -- an autograd function, used by ``FineTuneModelPool.forward`` so that
  ``model(x)`` / ``criterion(out, target)`` / ``loss.backward()`` of train.py:434-439 work unchanged;
* :meth:`NativeHead.loss_and_grad` -- logits, cross-entropy, and the whole backward of the head in 8 launches without
  autograd; ``Trainer.step`` takes this path when the criterion is a plain ``nn.CrossEntropyLoss`` or this package's
  ``MultiClassBCELoss`` (the multi-label branch: :meth:`NativeHead.bce`, csrc/mnas_mlabel.hip), ``MultiLabelLoss`` (that branch's
  asymmetric focal loss, pos_weight, smoothing and mixed label rows: :meth:`NativeHead.mlabel`), ``MixCrossEntropyLoss``
  (:meth:`NativeHead.cross_entropy_soft`) or ``DistillCrossEntropyLoss`` (class weights and a teacher's logits:
  :meth:`NativeHead.cross_entropy_kd`).

Dropout masks are a counter-based hash of (seed, element index) evaluated inside the GEMM kernels (never stored).  The seed
of a call is derived from ``torch.initial_seed()``, the rank and a per-head call counter, so runs are reproducible under
``torch.manual_seed`` but the mask stream is not ATen's Philox stream (the reference's masks differ from device to device
anyway).  No CPU fallback: tensors must live on the MI355X."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch
import torch.nn as nn

from . import _lib as L

_MASK64 = (1 << 64) - 1


def _mix(seed: int, a: int, b: int) -> int:
    """64-bit seed of (call, layer): splitmix64 finaliser, same arithmetic as oracle.head_layer_seed"""
    z = (seed + 0x9E3779B97F4A7C15 * (a + 1) + 0xD1B54A32D192ED03 * (b + 1)) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


class _Layer:
    __slots__ = ("p", "lin", "relu")

    def __init__(self, p, lin):
        self.p, self.lin, self.relu = p, lin, False


def parse_sequential(seq: nn.Module) -> Optional[List[_Layer]]:
    """[Dropout?] Linear [ReLU] ... -> layers, or None if the module is anything else (the caller then keeps PyTorch)."""
    if not isinstance(seq, nn.Sequential):
        return None
    layers: List[_Layer] = []
    pending = 0.0
    prev = None
    for m in seq:
        if isinstance(m, nn.Dropout):
            if prev == "drop" or not (0.0 <= m.p < 1.0):
                return None
            pending, prev = float(m.p), "drop"
        elif isinstance(m, nn.Linear):
            layers.append(_Layer(pending, m))
            pending, prev = 0.0, "lin"
        elif isinstance(m, nn.ReLU):
            if prev != "lin":
                return None
            layers[-1].relu, prev = True, "relu"
        else:
            return None
    if not layers or prev == "drop" or layers[-1].relu:
        return None            # trailing Dropout / ReLU on the logits: not one of the reference's heads
    for a, b in zip(layers, layers[1:]):
        if a.lin.out_features != b.lin.in_features:
            return None
    return layers


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, head, x, *params):
        seeds = head.next_seeds()
        # forward-time facts the backward needs: the mode decides whether the dropout masks apply (the masks are never stored, the
        # backward re-derives them from the seeds), the version counters say whether the weights are still the forward's
        training = bool(head.owner.training)
        us, logits = head.forward_layers(x, seeds, training)
        ctx.head, ctx.seeds, ctx.us, ctx.training = head, seeds, us, training
        ctx.versions = tuple(p._version for p in head.params())
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        head = ctx.head
        for (name, p), v in zip(head.named_params(), ctx.versions):
            if p._version != v:
                raise RuntimeError("classifier parameter %s was modified in place between a forward and its backward: the head's "
                                   "input gradient would use the new weights; run the forward again" % name)
        grads = [(torch.empty_like(l.lin.weight), torch.empty_like(l.lin.bias) if l.lin.bias is not None else None)
                 for l in head.layers]
        dx = head.backward_layers(ctx.us, ctx.seeds, dlogits.contiguous().float(), grads, accumulate=False,
                                  need_dx=ctx.needs_input_grad[1], training=ctx.training)
        flat = []
        for (dw, db), l in zip(grads, head.layers):
            flat.append(dw)
            if l.lin.bias is not None:
                flat.append(db)
        return (None, dx) + tuple(flat)


class NativeHead:
    def __init__(self, layers: List[_Layer], owner: nn.Module):
        self.layers = layers
        self.owner = owner               # the nn.Sequential: .training decides whether dropout is applied
        self.lib = L.load()
        self.calls = 0
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        self.seed0 = _mix(torch.initial_seed() & _MASK64, rank, 0x48454144)
        self._scratch = {}
        self._kd_rows = {}               # (N, device) -> the 2 N loss rows of cross_entropy_kd

    @staticmethod
    def build(seq: nn.Module) -> Optional["NativeHead"]:
        layers = parse_sequential(seq)
        return NativeHead(layers, seq) if layers is not None else None

    def params(self):
        out = []
        for l in self.layers:
            out.append(l.lin.weight)
            if l.lin.bias is not None:
                out.append(l.lin.bias)
        return out

    def named_params(self):
        """(name, parameter) in the order of params(); the name is the Linear's index in the layer list"""
        out = []
        for i, l in enumerate(self.layers):
            out.append(("linear[%d].weight" % i, l.lin.weight))
            if l.lin.bias is not None:
                out.append(("linear[%d].bias" % i, l.lin.bias))
        return out

    def next_seeds(self) -> List[int]:
        self.calls += 1
        return [_mix(self.seed0, self.calls, i) for i in range(len(self.layers))]

    # ---- kernels ----------------------------------------------------------------------------------------------------
    def _check(self, x):
        if x.device.type != "cuda":
            raise RuntimeError("the native head runs on the MI355X only (no CPU path)")
        if x.dim() != 2 or x.shape[1] != self.layers[0].lin.in_features:
            raise ValueError("head input must be (N, %d), got %s" % (self.layers[0].lin.in_features, tuple(x.shape)))

    def _desc(self, l: _Layer, N: int, seed: int, training: Optional[bool] = None) -> L.MnasHeadLinear:
        """training: the mode of the forward this descriptor belongs to (None: the owner's mode now)"""
        a = L.MnasHeadLinear()
        a.N, a.I, a.O = N, l.lin.in_features, l.lin.out_features
        a.relu = 1 if l.relu else 0
        a.drop_p = l.p if (self.owner.training if training is None else training) else 0.0
        a.seed = seed
        a.w = l.lin.weight.data_ptr()
        a.b = L.ptr(l.lin.bias)
        return a

    def forward_layers(self, x, seeds, training: Optional[bool] = None):
        """-> ([input of every layer], logits).  x: (N, I0) fp32 contiguous."""
        self._check(x)
        x = x.contiguous().float()
        N = x.shape[0]
        us = []
        for l, seed in zip(self.layers, seeds):
            if not (l.lin.weight.is_contiguous() and l.lin.weight.dtype == torch.float32):
                raise RuntimeError("head weights must be contiguous fp32")
            y = torch.empty((N, l.lin.out_features), dtype=torch.float32, device=x.device)
            a = self._desc(l, N, seed, training)
            a.x, a.y = x.data_ptr(), y.data_ptr()
            L.check(self.lib.mnas_head_linear_fwd(C.byref(a), L.cur_stream()), "head_linear_fwd")
            us.append(x)
            x = y
        return us, x

    def backward_layers(self, us, seeds, dz, grads, accumulate: bool, need_dx: bool = True, training: Optional[bool] = None):
        """dz: gradient of the logits.  grads[i] = (dW, db or None) tensors written (or accumulated into).  -> dx or None.
        training: the mode the forward ran in (its dropout masks apply again); None: the owner's mode now"""
        N = dz.shape[0]
        for i in range(len(self.layers) - 1, -1, -1):
            l = self.layers[i]
            a = self._desc(l, N, seeds[i], training)
            a.x, a.dz = us[i].data_ptr(), dz.data_ptr()
            a.dw, a.db = grads[i][0].data_ptr(), L.ptr(grads[i][1])
            a.accumulate = 1 if accumulate else 0
            L.check(self.lib.mnas_head_linear_bwd_w(C.byref(a), L.cur_stream()), "head_linear_bwd_w")
            if i == 0 and not need_dx:
                return None
            dx = torch.empty((N, l.lin.in_features), dtype=torch.float32, device=dz.device)
            a.dx = dx.data_ptr()
            a.relu_mask = us[i].data_ptr() if (i > 0 and self.layers[i - 1].relu) else None
            L.check(self.lib.mnas_head_linear_bwd_x(C.byref(a), L.cur_stream()), "head_linear_bwd_x")
            dz = dx
        return dz

    def cross_entropy(self, logits, target, ignore_index=-100, need_grad=True, meters=None):
        """-> (loss 0-d tensor, dlogits or None).  nn.CrossEntropyLoss(reduction='mean') semantics.  ``meters`` (a
        metrics.DeviceMeters): the same two launches also update its loss / top-k accuracy block (train.py:447,465-468)."""
        N, Cn = logits.shape
        if target.dtype != torch.int64 or target.shape != (N,):
            raise ValueError("target must be int64 of shape (N,)")
        if target.device != logits.device:
            raise RuntimeError("target is on %s, logits on %s (the kernel takes raw device pointers)" % (target.device, logits.device))
        dev = logits.device
        key = (N, dev)
        if key not in self._scratch:
            self._scratch[key] = (torch.empty(N, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        rows, bad = self._scratch[key]
        loss = torch.empty((), dtype=torch.float32, device=dev)
        dl = torch.empty_like(logits) if need_grad else None
        if meters is not None:
            ks, nk, ranks, blk = meters.kernel_args(N, dev)
            L.check(self.lib.mnas_head_cross_entropy_metrics(logits.data_ptr(), target.contiguous().data_ptr(), N, Cn, int(ignore_index),
                                                             rows.data_ptr(), loss.data_ptr(), L.ptr(dl), bad.data_ptr(), ks, nk,
                                                             ranks, blk, L.cur_stream()), "head_cross_entropy_metrics")
            return loss, dl
        L.check(self.lib.mnas_head_cross_entropy(logits.data_ptr(), target.contiguous().data_ptr(), N, Cn, int(ignore_index),
                                                 rows.data_ptr(), loss.data_ptr(), L.ptr(dl), bad.data_ptr(), L.cur_stream()),
                "head_cross_entropy")
        return loss, dl

    def cross_entropy_soft(self, logits, target, label_smoothing=0.0, ignore_index=-100, need_grad=True, meters=None):
        """-> (loss 0-d tensor, dlogits or None) of a losses.MixCrossEntropyLoss: cross-entropy with label smoothing over an int64
        class vector or a mixing.MixedTarget (two labels and a weight per row).  ``meters`` (a metrics.DeviceMeters): the same two
        launches move its block, every row ranked against its heavier label.  A plain class vector without smoothing runs
        :meth:`cross_entropy`'s launches (same arithmetic, bit for bit what nn.CrossEntropyLoss() steps)."""
        from .losses import soft_cross_entropy, split_target
        a, b, lam = split_target(target)
        if b is None and float(label_smoothing) == 0.0:
            return self.cross_entropy(logits, a, ignore_index, need_grad=need_grad, meters=meters)
        N, dev = logits.shape[0], logits.device
        if b is not None:
            target.check_device(dev)
        key = (N, dev)
        if key not in self._scratch:
            self._scratch[key] = (torch.empty(N, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        rows, bad = self._scratch[key]
        return soft_cross_entropy(logits, a, b, lam, label_smoothing, ignore_index, rows=rows, bad=bad, need_grad=need_grad, meters=meters)

    def cross_entropy_kd(self, logits, target, criterion, need_grad=True, meters=None):
        """-> (loss 0-d tensor, dlogits or None) of a losses.DistillCrossEntropyLoss ``criterion``: class weights, label smoothing
        and the distillation term in two launches (mnas_head_cross_entropy_kd).  ``target``: a class vector, a mixing.MixedTarget
        or a losses.DistillTarget around either (only that one carries teacher logits).  Without a weight and without a teacher
        it is :meth:`cross_entropy_soft` (and through it the plain kernel): such a criterion steps bit for bit like a
        MixCrossEntropyLoss or an nn.CrossEntropyLoss with the same settings.  ``criterion.last_parts`` names (hard, kd) on the
        device afterwards (None after the fall-through case, which has no parts)."""
        from .losses import DistillTarget, kd_cross_entropy, split_distill_target
        N, dev = logits.shape[0], logits.device
        if isinstance(target, DistillTarget):
            target.check_device(dev)
        a, b, lam, teacher = split_distill_target(target)
        weight = criterion.class_weight(logits)
        if weight is None and teacher is None:
            plain = target.target if isinstance(target, DistillTarget) else target
            criterion.last_parts = None
            return self.cross_entropy_soft(logits, plain, criterion.label_smoothing, criterion.ignore_index, need_grad=need_grad,
                                           meters=meters)
        if b is not None:
            (target.target if isinstance(target, DistillTarget) else target).check_device(dev)
        key = (N, dev)
        if key not in self._kd_rows:
            self._kd_rows[key] = torch.empty(2 * N, dtype=torch.float32, device=dev)
        bad, parts = criterion.buffers_for(dev)
        return kd_cross_entropy(logits, a, b, lam, criterion.label_smoothing, weight, teacher, criterion.temperature, criterion.alpha,
                                criterion.ignore_index, rows=self._kd_rows[key], bad=bad, parts=parts, need_grad=need_grad, meters=meters)

    def bce(self, logits, target, criterion, weights=None, need_grad=True, meters=None, f1_n=None):
        """-> (loss 0-d tensor, dlogits or None) of a losses.MultiClassBCELoss ``criterion`` (csrc/mnas_mlabel.hip).  target: (N, C),
        converted with .float() as train.py:429 does.  ``meters`` (a metrics.MultiLabelMeters): the same launches also update its
        loss / HardDice(0.5) / F1 block with the weights N, N and ``f1_n`` (default N)."""
        from .losses import bce_with_logits
        N = logits.shape[0]
        if not isinstance(target, torch.Tensor) or target.shape != logits.shape:
            raise ValueError("multi-label target must be of shape (N, C) = %s, got %s"
                             % (tuple(logits.shape), tuple(getattr(target, "shape", ()))))
        target, weights = criterion.prepare(logits, target, weights)
        return bce_with_logits(logits, target, weights, bool(criterion.use_focal_weights), criterion.focus_param,
                               criterion.balance_param, need_grad=need_grad, meters=meters,
                               meter_weights=(N, N, N if f1_n is None else f1_n))

    def mlabel(self, logits, target, criterion, weights=None, need_grad=True, meters=None, f1_n=None):
        """-> (loss 0-d tensor, dlogits or None) of a losses.MultiLabelLoss ``criterion`` (mnas_mlabel_loss: asymmetric focusing,
        pos_weight, smoothing, two launches).  target: an (N, C) label matrix (converted with .float()) or a mixing.MixedLabels,
        whose rows are mixed on load.  ``meters`` (a metrics.MultiLabelMeters): the same launches also update its block with the
        weights N, N and ``f1_n`` (default N), every row counted against its dominant image's labels."""
        from .losses import multilabel_loss
        N = logits.shape[0]
        labels, partner, lam, weights, pw = criterion.prepare(logits, target, weights)
        return multilabel_loss(logits, labels, partner, lam, weights, pw, *criterion.settings(), need_grad=need_grad, meters=meters,
                               meter_weights=(N, N, N if f1_n is None else f1_n))

    def check_targets(self):
        """Host check of the device-side "target out of range" flag that mnas_head_cross_entropy raises (the loss is NaN from
        that step on; ATen asserts on the device instead).  Synchronises: call it next to a ``loss.item()``, not per step.
        Resets the flag."""
        for (N, dev), (_, bad) in self._scratch.items():
            if int(bad.item()) != 0:
                bad.zero_()
                raise ValueError("cross_entropy: a target index was outside [0, num_classes) and not ignore_index "
                                 "(or, for a mixed batch, a weight outside [0, 1])")

    # ---- entry points -----------------------------------------------------------------------------------------------
    def apply(self, x):
        return _HeadFn.apply(self, x, *self.params())

    def loss_and_grad(self, x, target, ignore_index=-100, need_dx=True, meters=None, criterion=None, f1_n=None):
        """Forward, loss and full backward of the head without autograd.  Parameter gradients are ACCUMULATED into
        ``p.grad`` (which must exist: Trainer points them into its flat gradient buffer).  -> (logits, loss, dx).
        ``criterion``: None / an nn.CrossEntropyLoss -> cross-entropy with ``ignore_index``; a losses.MultiClassBCELoss -> :meth:`bce`;
        a losses.MultiLabelLoss -> :meth:`mlabel` (``target``: a label matrix or a mixing.MixedLabels); a losses.MixCrossEntropyLoss -> :meth:`cross_entropy_soft` (``target``: a class vector or a mixing.MixedTarget); a
        losses.DistillCrossEntropyLoss -> :meth:`cross_entropy_kd` (``target``: either of those, or a losses.DistillTarget)."""
        from .losses import DistillCrossEntropyLoss, MixCrossEntropyLoss, MultiClassBCELoss, MultiLabelLoss
        seeds = self.next_seeds()
        us, logits = self.forward_layers(x, seeds)
        if type(criterion) is MultiClassBCELoss:             # the class itself, as Trainer routes it
            loss, dl = self.bce(logits, target, criterion, meters=meters, f1_n=f1_n)
        elif type(criterion) is MultiLabelLoss:
            loss, dl = self.mlabel(logits, target, criterion, meters=meters, f1_n=f1_n)
        elif type(criterion) is MixCrossEntropyLoss:
            loss, dl = self.cross_entropy_soft(logits, target, criterion.label_smoothing, criterion.ignore_index, meters=meters)
        elif type(criterion) is DistillCrossEntropyLoss:
            loss, dl = self.cross_entropy_kd(logits, target, criterion, meters=meters)
        else:
            loss, dl = self.cross_entropy(logits, target, ignore_index, meters=meters)
        grads = []
        for l in self.layers:
            if l.lin.weight.grad is None or (l.lin.bias is not None and l.lin.bias.grad is None):
                raise RuntimeError("loss_and_grad needs preallocated .grad tensors on the head parameters")
            grads.append((l.lin.weight.grad, l.lin.bias.grad if l.lin.bias is not None else None))
        dx = self.backward_layers(us, seeds, dl, grads, accumulate=True, need_dx=need_dx)
        return logits, loss, dx

    def dropout_mask(self, layer: int, N: int, seed: int):
        """keep mask (N, in_features) uint8 of one layer for a given seed (tests)."""
        l = self.layers[layer]
        out = torch.empty((N, l.lin.in_features), dtype=torch.uint8, device="cuda")
        L.check(self.lib.mnas_head_dropout_mask(out.data_ptr(), out.numel(), l.p, seed, L.cur_stream()), "head_dropout_mask")
        return out
