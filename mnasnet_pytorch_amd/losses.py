"""The criterion and the Dice metric of the reference's multi-label branch (``src/models/multi_class_loss.py``; train.py:274-279
builds ``MultiClassBCELoss()`` and ``HardDice(threshold=0.5)`` when ``--multi_class`` is set, its default) on the HIP library
(csrc/mnas_mlabel.hip; the arithmetic rule is stated in include/mnas.h).

* :class:`MultiClassBCELoss` -- same constructor and ``forward(outputs, targets, weights=None)``.  BCE-with-logits, mean-reduced,
  optional element weights, optional focal transform of the MEAN (as the reference applies it).  Differentiable with respect to
  ``outputs``.  ``Trainer`` recognises this class and runs the whole step without autograd (head.NativeHead.bce).
* :class:`MultiLabelLoss` -- not from the reference: that branch's current recipe in the same two launches -- per-element asymmetric
  focal loss, ``pos_weight``, binary label smoothing, and label rows mixed on load from a ``mixing.MixedLabels`` (include/mnas.h
  "multi-label loss"; head.NativeHead.mlabel).  ``Trainer`` recognises this class too; :func:`multilabel_loss` is the functional form.
* :class:`HardDice` -- same constructor; returns a 0-d fp32 device tensor without a host sync.
* :class:`MixCrossEntropyLoss` -- not from the reference: cross-entropy with label smoothing over class indices or over the two
  labels per row of a mixed batch (mixing.MixedTarget; csrc/mnas_head.hip, include/mnas.h "soft-target cross-entropy").  ``Trainer``
  recognises this class too (head.NativeHead.cross_entropy_soft).
* :class:`DistillCrossEntropyLoss` / :class:`DistillTarget` -- not from the reference either: class weights, label smoothing and a
  knowledge-distillation term against a teacher's logits in the same two launches (include/mnas.h "distillation cross-entropy";
  head.NativeHead.cross_entropy_kd).  ``Trainer(teacher=...)`` runs the teacher's forward and wraps the target.

Deviations: the Dice prediction is ``outputs > logit(threshold)`` instead of ``sigmoid(outputs) > threshold`` (equal except where
the fp32 sigmoid rounds onto the threshold), so the threshold must lie inside (0, 1); ``focus_param < 1`` is refused (the gradient
holds ``(1 - pt) ** (focus_param - 1)``).  No CPU path: tensors must live on the MI355X."""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from . import _lib as L


def _scratch(lib, N, device):
    return torch.empty(int(lib.mnas_mlabel_scratch_bytes(N)), dtype=torch.uint8, device=device)


def _on_device(name, t, device=None):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError("%s must be a tensor on the MI355X (no CPU path)" % name)
    if device is not None and t.device != device:
        raise RuntimeError("%s is on %s, outputs on %s (the kernels take raw device pointers)" % (name, t.device, device))


def check_focus_param(focus_param):
    if not float(focus_param) >= 1.0:
        raise ValueError("focus_param must be >= 1 (the gradient holds (1 - pt) ** (focus_param - 1)), got %r" % (focus_param,))


def bce_with_logits(logits, target, weights=None, focal=False, focus_param=2, balance_param=0.25, need_grad=True, meters=None,
                    meter_weights=None):
    """mnas_mlabel_bce on (N, C) fp32 contiguous device tensors -> (loss 0-d tensor, dlogits or None).  ``meters`` (a
    metrics.MultiLabelMeters) with ``meter_weights = (n_loss, n_dice, n_f1)``: the same launches also move its block."""
    lib = L.load()
    N, Cn = logits.shape
    dev = logits.device
    if focal:
        check_focus_param(focus_param)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if need_grad else None
    scratch = _scratch(lib, N, dev)
    blk, (n_loss, n_dice, n_f1) = 0, (0, 0, 0)
    if meters is not None:
        blk = meters.kernel_args(dev)
        n_loss, n_dice, n_f1 = (int(v) for v in meter_weights)
    L.check(lib.mnas_mlabel_bce(logits.data_ptr(), target.data_ptr(), L.ptr(weights), N, Cn, 1 if focal else 0, float(focus_param),
                                float(balance_param), scratch.data_ptr(), loss.data_ptr(), L.ptr(dl), blk, n_loss, n_dice, n_f1,
                                L.cur_stream()), "mlabel_bce")
    return loss, dl


class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, targets, weights, focal, focus_param, balance_param):
        loss, dl = bce_with_logits(outputs.detach().float().contiguous(), targets, weights, focal, focus_param, balance_param,
                                   need_grad=ctx.needs_input_grad[0])
        ctx.dl, ctx.dtype = dl, outputs.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        return (ctx.dl * grad_output).to(ctx.dtype), None, None, None, None, None


class MultiClassBCELoss(nn.Module):
    def __init__(self, use_weight_mask=False, use_focal_weights=False, focus_param=2, balance_param=0.25):
        super().__init__()
        self.use_weight_mask = use_weight_mask
        self.use_focal_weights = use_focal_weights
        self.focus_param = focus_param
        self.balance_param = balance_param
        if use_focal_weights:
            check_focus_param(focus_param)

    def prepare(self, outputs, targets, weights=None):
        """shape and device checks -> (targets, weights or None) as fp32 contiguous tensors.  A target whose rank, row count or
        class count differs from the outputs' is an AssertionError, as it is for the reference's criterion; the weights are
        dropped unless use_weight_mask is set, as there"""
        if outputs.dim() != 2:
            raise ValueError("outputs must be (N, C), got %s" % (tuple(outputs.shape),))
        N, Cn = outputs.shape
        assert targets.dim() == 2, "targets have %d dimensions, outputs 2" % targets.dim()
        assert targets.shape[0] == N, "targets have %d rows, outputs %d" % (targets.shape[0], N)
        assert targets.shape[1] == Cn, "targets have %d classes, outputs %d" % (targets.shape[1], Cn)
        if weights is not None and weights.shape != outputs.shape:
            raise ValueError("weights must be %s, got %s" % (tuple(outputs.shape), tuple(weights.shape)))
        _on_device("outputs", outputs)
        _on_device("targets", targets, outputs.device)
        targets = targets.detach().float().contiguous()
        if weights is not None and self.use_weight_mask:
            _on_device("weights", weights, outputs.device)
            weights = weights.detach().float().contiguous()
        else:
            weights = None
        return targets, weights

    def forward(self, outputs, targets, weights=None):
        targets, weights = self.prepare(outputs, targets, weights)
        return _BCEFn.apply(outputs, targets, weights, bool(self.use_focal_weights), self.focus_param, self.balance_param)


REDUCTIONS = {"mean": L.MLABEL_MEAN, "rows": L.MLABEL_ROWS}


def check_multilabel_settings(gamma_pos, gamma_neg, margin, label_smoothing, reduction):
    """the ranges mnas_mlabel_loss accepts (include/mnas.h "multi-label loss"), as ValueErrors"""
    for name, g in (("gamma_pos", gamma_pos), ("gamma_neg", gamma_neg)):
        g = float(g)
        if not (g == 0.0 or 1.0 <= g <= 16.0):
            raise ValueError("%s must be 0 or lie in [1, 16] (the gradient holds the focusing weight to the power gamma - 1), got %r"
                             % (name, g))
    if not 0.0 <= float(margin) <= 0.5:
        raise ValueError("margin must lie in [0, 0.5], got %r" % (margin,))
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError("label_smoothing must lie in [0, 1), got %r" % (label_smoothing,))
    if reduction not in REDUCTIONS:
        raise ValueError("reduction must be 'mean' (over N*C) or 'rows' (summed over the classes, averaged over the rows), got %r"
                         % (reduction,))


def split_labels(target):
    """an (N, C) label matrix or a mixing.MixedLabels -> (labels, partner or None, lam or None)"""
    from .mixing import MixedLabels
    if isinstance(target, MixedLabels):
        return target.labels, target.partner, target.lam
    return target, None, None


def multilabel_loss(logits, labels, partner=None, lam=None, weights=None, pos_weight=None, gamma_pos=0.0, gamma_neg=0.0, margin=0.0,
                    label_smoothing=0.0, reduction="mean", need_grad=True, meters=None, meter_weights=None):
    """mnas_mlabel_loss on (N, C) fp32 contiguous device tensors -> (loss 0-d tensor, dlogits or None): the asymmetric focal loss
    with ``pos_weight`` (fp32 (C,)), binary label smoothing and, with ``partner`` (int64 (N,)) and ``lam`` (fp32 (N,)), label rows
    mixed on load.  ``meters`` (a metrics.MultiLabelMeters) with ``meter_weights = (n_loss, n_dice, n_f1)``: the same launches also
    move its block, every row counted against its dominant image's labels."""
    _on_device("logits", logits)
    if logits.dim() != 2:
        raise ValueError("logits must be (N, C), got %s" % (tuple(logits.shape),))
    N, Cn = logits.shape
    dev = logits.device
    if (partner is None) != (lam is None):
        raise ValueError("partner and lam come together (a mixing.MixedLabels holds both)")
    for name, t, dt, shape in (("logits", logits, torch.float32, (N, Cn)), ("labels", labels, torch.float32, (N, Cn)),
                               ("partner", partner, torch.int64, (N,)), ("lam", lam, torch.float32, (N,)),
                               ("weights", weights, torch.float32, (N, Cn)), ("pos_weight", pos_weight, torch.float32, (Cn,))):
        if t is None:
            continue
        _on_device(name, t, dev)
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("%s must be contiguous %s of shape %s, got %s %s" % (name, dt, shape, t.dtype, tuple(t.shape)))
    check_multilabel_settings(gamma_pos, gamma_neg, margin, label_smoothing, reduction)
    lib = L.load()
    cfg = L.MnasMlabelLoss(float(gamma_pos), float(gamma_neg), float(margin), float(label_smoothing), REDUCTIONS[reduction])
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if need_grad else None
    scratch = _scratch(lib, N, dev)
    blk, (n_loss, n_dice, n_f1) = 0, (0, 0, 0)
    if meters is not None:
        blk = meters.kernel_args(dev)
        n_loss, n_dice, n_f1 = (int(v) for v in meter_weights)
    L.check(lib.mnas_mlabel_loss(logits.data_ptr(), labels.data_ptr(), L.ptr(partner), L.ptr(lam), L.ptr(weights), L.ptr(pos_weight),
                                 N, Cn, ctypes.byref(cfg), scratch.data_ptr(), loss.data_ptr(), L.ptr(dl), blk, n_loss, n_dice, n_f1,
                                 L.cur_stream()), "mlabel_loss")
    return loss, dl


class _MLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, labels, partner, lam, weights, pos_weight, settings):
        loss, dl = multilabel_loss(outputs.detach().float().contiguous(), labels, partner, lam, weights, pos_weight, *settings,
                                   need_grad=ctx.needs_input_grad[0])
        ctx.dl, ctx.dtype = dl, outputs.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        return (ctx.dl * grad_output).to(ctx.dtype), None, None, None, None, None, None


class MultiLabelLoss(nn.Module):
    """The multi-label branch's current recipe in the BCE loss's two launches (not from the reference; include/mnas.h "multi-label
    loss"): the asymmetric focal loss of Ridnik et al. -- per ELEMENT, the focusing weights differentiated --

        e = w * ( pos_weight_c * t * (1 - s)^gamma_pos * -log(s)  +  (1 - t) * s_m^gamma_neg * -log(1 - s_m) ),
        s = sigmoid(z),  s_m = max(s - margin, 0),  t = (1 - label_smoothing) * y + label_smoothing / 2

    ``gamma_pos = gamma_neg = gamma, margin = 0`` is the sigmoid focal loss without its alpha term; everything 0 is
    ``F.binary_cross_entropy_with_logits(weight=, pos_weight=)``.  ``reduction``: ``"mean"`` over N*C, or ``"rows"`` -- summed over
    the classes, averaged over the rows.  ``forward(outputs, targets, weights=None)``: ``targets`` an ``(N, C)`` label matrix
    (soft values allowed; integer matrices are converted with ``.float()``) or a ``mixing.MixedLabels``, whose rows are mixed on
    load; ``weights`` (``(N, C)``) are dropped unless ``use_weight_mask`` is set, as for :class:`MultiClassBCELoss`.
    ``pos_weight``: a registered buffer ``(C,)`` (it moves with ``.to()`` / ``.cuda()``) or None.  Differentiable with respect to
    ``outputs`` only.  ``Trainer`` recognises this class and runs the whole step without autograd (head.NativeHead.mlabel).  A row
    whose partner index or weight is out of range makes the loss and its gradient row NaN.  With a margin the negative part is
    computed from the rounded sigmoid, ``-log1p(-(s - margin))``: it is capped at ``-log(margin)``, and a margin below 2**-24
    (other than 0) would make it infinite where the sigmoid rounds to 1 -- use 0 or a real margin.  No CPU path."""

    def __init__(self, gamma_pos: float = 0.0, gamma_neg: float = 0.0, margin: float = 0.0, pos_weight=None, label_smoothing: float = 0.0,
                 use_weight_mask: bool = False, reduction: str = "mean"):
        super().__init__()
        check_multilabel_settings(gamma_pos, gamma_neg, margin, label_smoothing, reduction)
        self.gamma_pos, self.gamma_neg, self.margin = float(gamma_pos), float(gamma_neg), float(margin)
        self.label_smoothing, self.use_weight_mask, self.reduction = float(label_smoothing), bool(use_weight_mask), reduction
        self.register_buffer("pos_weight", check_class_weight(pos_weight))

    def settings(self):
        return (self.gamma_pos, self.gamma_neg, self.margin, self.label_smoothing, self.reduction)

    def prepare(self, outputs, targets, weights=None):
        """shape and device checks -> (labels, partner or None, lam or None, weights or None, pos_weight or None), the tensors
        fp32 / int64 contiguous on the outputs' device"""
        from .mixing import MixedLabels
        if not isinstance(outputs, torch.Tensor) or outputs.dim() != 2:
            raise ValueError("outputs must be (N, C), got %s" % (tuple(getattr(outputs, "shape", ())),))
        _on_device("outputs", outputs)
        if isinstance(targets, MixedLabels):
            targets.check_device(outputs.device)
        labels, partner, lam = split_labels(targets)
        if not isinstance(labels, torch.Tensor) or labels.shape != outputs.shape:
            raise ValueError("targets must be an (N, C) = %s label matrix or a MixedLabels around one, got %s"
                             % (tuple(outputs.shape), tuple(getattr(labels, "shape", ()))))
        if weights is not None and weights.shape != outputs.shape:
            raise ValueError("weights must be %s, got %s" % (tuple(outputs.shape), tuple(weights.shape)))
        _on_device("targets", labels, outputs.device)
        labels = labels.detach().float().contiguous()
        if weights is not None and self.use_weight_mask:
            _on_device("weights", weights, outputs.device)
            weights = weights.detach().float().contiguous()
        else:
            weights = None
        pw = self.pos_weight
        if pw is not None:
            if pw.numel() != outputs.shape[1]:
                raise ValueError("pos_weight has %d entries, the outputs %d classes" % (pw.numel(), outputs.shape[1]))
            _on_device("pos_weight", pw, outputs.device)
        return labels, partner, lam, weights, pw

    def forward(self, outputs, targets, weights=None):
        labels, partner, lam, weights, pw = self.prepare(outputs, targets, weights)
        return _MLFn.apply(outputs, labels, partner, lam, weights, pw, self.settings())

    def extra_repr(self):
        return "gamma_pos=%g, gamma_neg=%g, margin=%g, label_smoothing=%g, pos_weight=%s, reduction=%r" % (
            self.gamma_pos, self.gamma_neg, self.margin, self.label_smoothing,
            "None" if self.pos_weight is None else "(%d,)" % self.pos_weight.numel(), self.reduction)


def soft_cross_entropy(logits, a, b=None, lam=None, label_smoothing=0.0, ignore_index=-100, rows=None, bad=None, need_grad=True,
                       meters=None):
    """mnas_head_cross_entropy_soft on (N, C) fp32 contiguous device logits -> (loss 0-d tensor, dlogits or None).  ``a``: int64 (N,);
    ``b`` / ``lam``: the second label and the weight of ``a`` per row (int64 / fp32 (N,)), or None for no mixing.  ``rows`` / ``bad``:
    the fp32 (N,) scratch and the int32 "target refused" flag (allocated when not given).  ``meters`` (a metrics.DeviceMeters): the
    same two launches also move its block, every row ranked against its heavier label."""
    lib = L.load()
    N, Cn = logits.shape
    dev = logits.device
    for name, t, dt in (("target", a, torch.int64), ("second target", b, torch.int64), ("lam", lam, torch.float32)):
        if t is None:
            continue
        _on_device(name, t, dev)
        if t.dtype != dt or t.shape != (N,):
            raise ValueError("%s must be %s of shape (N,) = (%d,), got %s %s" % (name, dt, N, t.dtype, tuple(t.shape)))
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError("label_smoothing must lie in [0, 1], got %r" % (label_smoothing,))
    if rows is None:
        rows = torch.empty(N, dtype=torch.float32, device=dev)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if need_grad else None
    ks, nk, ranks, blk = (None, 0, 0, 0) if meters is None else meters.kernel_args(N, dev)
    L.check(lib.mnas_head_cross_entropy_soft(logits.data_ptr(), a.contiguous().data_ptr(), L.ptr(None if b is None else b.contiguous()),
                                             L.ptr(None if lam is None else lam.contiguous()), eps, N, Cn, int(ignore_index),
                                             rows.data_ptr(), loss.data_ptr(), L.ptr(dl), bad.data_ptr(), ks, nk, ranks, blk,
                                             L.cur_stream()), "head_cross_entropy_soft")
    return loss, dl


def split_target(target):
    """a class vector or a mixing.MixedTarget -> (a, b or None, lam or None)"""
    from .mixing import MixedTarget
    if isinstance(target, MixedTarget):
        return target.a, target.b, target.lam
    return target, None, None


class _SoftCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, a, b, lam, label_smoothing, ignore_index, bad):
        loss, dl = soft_cross_entropy(logits.detach().float().contiguous(), a, b, lam, label_smoothing, ignore_index, bad=bad,
                                      need_grad=ctx.needs_input_grad[0])
        ctx.dl, ctx.dtype = dl, logits.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        return (ctx.dl * grad_output).to(ctx.dtype), None, None, None, None, None, None


class MixCrossEntropyLoss(nn.Module):
    """Mean cross-entropy with label smoothing over class indices (int64 ``(N,)``) or over a mixed batch's two labels per row (a
    ``mixing.MixedTarget``): per row ``lam CE(a) + (1 - lam) CE(b)`` with ``CE = F.cross_entropy(..., label_smoothing)``, averaged
    over the rows whose labels are not ``ignore_index``.  Differentiable with respect to the logits.  ``Trainer`` recognises this
    class and runs the whole step without autograd.  No class weights.  No CPU path."""

    def __init__(self, label_smoothing: float = 0.0, ignore_index: int = -100):
        super().__init__()
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError("label_smoothing must lie in [0, 1], got %r" % (label_smoothing,))
        self.label_smoothing = float(label_smoothing)
        self.ignore_index = int(ignore_index)
        self._bad = {}                   # device -> int32 flag raised by a refused label or weight

    def forward(self, logits, target):
        _on_device("logits", logits)
        if logits.dim() != 2:
            raise ValueError("logits must be (N, C), got %s" % (tuple(logits.shape),))
        a, b, lam = split_target(target)
        _on_device("target", a, logits.device)
        bad = self._bad.get(logits.device)
        if bad is None:
            bad = self._bad[logits.device] = torch.zeros(1, dtype=torch.int32, device=logits.device)
        return _SoftCEFn.apply(logits, a, b, lam, self.label_smoothing, self.ignore_index, bad)

    def check_targets(self):
        """Host check of the device-side flag a label outside [0, C) or a weight outside [0, 1] raises (the loss is NaN from that
        call on).  Synchronises; resets the flag."""
        for bad in self._bad.values():
            if int(bad.item()) != 0:
                bad.zero_()
                raise ValueError("MixCrossEntropyLoss: a label was outside [0, num_classes) and not ignore_index, or a weight outside [0, 1]")

    def extra_repr(self):
        return "label_smoothing=%g, ignore_index=%d" % (self.label_smoothing, self.ignore_index)


class DistillTarget:
    """The target of a distilled step: ``target`` -- an int64 class vector ``(N,)`` or a ``mixing.MixedTarget`` -- together with the
    teacher's logits ``(N, C)`` fp32 for the same rows, all on one MI355X device.  ``Trainer(teacher=...)`` builds it from the
    teacher's forward; build it by hand for cached teacher logits.  No gradient flows to the teacher logits."""

    def __init__(self, target, teacher_logits: torch.Tensor):
        from .mixing import MixedTarget
        if isinstance(target, DistillTarget):
            raise TypeError("DistillTarget.target must be a class vector or a MixedTarget, not another DistillTarget")
        if not isinstance(target, MixedTarget):
            if not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or target.dim() != 1:
                raise TypeError("DistillTarget.target must be a 1-D int64 class vector or a mixing.MixedTarget")
        if not isinstance(teacher_logits, torch.Tensor) or teacher_logits.dtype != torch.float32 or teacher_logits.dim() != 2:
            raise TypeError("DistillTarget.teacher_logits must be a 2-D fp32 tensor (N, C)")
        if teacher_logits.shape[0] != target.shape[0]:
            raise ValueError("the target has %d rows, the teacher logits %d" % (target.shape[0], teacher_logits.shape[0]))
        if teacher_logits.device != target.device:
            raise RuntimeError("target and teacher logits must be on one device, got %s and %s" % (target.device, teacher_logits.device))
        self.target, self.teacher_logits = target, teacher_logits.detach().contiguous()

    @property
    def device(self):
        return self.teacher_logits.device

    @property
    def shape(self):
        return self.target.shape

    def __len__(self):
        return self.target.shape[0]

    def to(self, device, non_blocking: bool = False) -> "DistillTarget":
        return DistillTarget(self.target.to(device, non_blocking=non_blocking), self.teacher_logits.to(device, non_blocking=non_blocking))

    def check_device(self, device):
        """the kernels take raw device pointers: everything on ``device``, an MI355X"""
        if self.device.type != "cuda":
            raise RuntimeError("a DistillTarget must be on the MI355X (no CPU path)")
        if self.device != torch.device(device):
            raise RuntimeError("the DistillTarget is on %s, the logits on %s (the kernels take raw device pointers)" % (self.device, device))

    def __repr__(self):
        return "DistillTarget(N=%d, C=%d, device=%s)" % (len(self), self.teacher_logits.shape[1], self.device)


def split_distill_target(target):
    """a class vector, a mixing.MixedTarget or a DistillTarget around either -> (a, b or None, lam or None, teacher logits or None)"""
    teacher = None
    if isinstance(target, DistillTarget):
        target, teacher = target.target, target.teacher_logits
    return split_target(target) + (teacher,)


def check_class_weight(weight):
    """class weights: a 1-D tensor of finite values >= 0 (the kernel does not check them) -> fp32 contiguous, or None"""
    if weight is None:
        return None
    if not isinstance(weight, torch.Tensor) or weight.dim() != 1 or weight.numel() < 1:
        raise ValueError("weight must be a 1-D tensor with one entry per class, got %s"
                         % (tuple(weight.shape) if isinstance(weight, torch.Tensor) else type(weight).__name__,))
    weight = weight.detach().float().contiguous()
    if not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
        raise ValueError("class weights must be finite and >= 0")
    return weight


def kd_cross_entropy(logits, a, b=None, lam=None, label_smoothing=0.0, weight=None, teacher=None, temperature=1.0, alpha=0.5,
                     ignore_index=-100, rows=None, bad=None, parts=None, need_grad=True, meters=None):
    """mnas_head_cross_entropy_kd on (N, C) fp32 contiguous device logits -> (loss 0-d tensor, dlogits or None).  ``a`` / ``b`` /
    ``lam`` as for :func:`soft_cross_entropy`; ``weight``: fp32 (C,) class weights or None; ``teacher``: fp32 (N, C) teacher logits
    or None (then the loss is the hard term alone).  ``rows``: the fp32 (2 N,) scratch (hard and distillation rows), ``bad``: the
    int32 "target refused" flag, ``parts``: fp32 (2,) receiving (hard, kd) -- each allocated when not given."""
    lib = L.load()
    N, Cn = logits.shape
    dev = logits.device
    for name, t, dt, shape in (("target", a, torch.int64, (N,)), ("second target", b, torch.int64, (N,)), ("lam", lam, torch.float32, (N,)),
                               ("weight", weight, torch.float32, (Cn,)), ("teacher logits", teacher, torch.float32, (N, Cn))):
        if t is None:
            continue
        _on_device(name, t, dev)
        if t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError("%s must be %s of shape %s, got %s %s" % (name, dt, shape, t.dtype, tuple(t.shape)))
    eps, T, al = float(label_smoothing), float(temperature), float(alpha)
    check_distill_settings(T, al, eps)
    if rows is None:
        rows = torch.empty(2 * N, dtype=torch.float32, device=dev)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if parts is None:
        parts = torch.empty(2, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if need_grad else None
    ks, nk, ranks, blk = (None, 0, 0, 0) if meters is None else meters.kernel_args(N, dev)
    cont = lambda t: None if t is None else t.contiguous()
    a, b, lam, weight, teacher = (cont(t) for t in (a, b, lam, weight, teacher))
    L.check(lib.mnas_head_cross_entropy_kd(logits.data_ptr(), a.data_ptr(), L.ptr(b), L.ptr(lam), eps, L.ptr(weight), L.ptr(teacher), T, al,
                                           N, Cn, int(ignore_index), rows.data_ptr(), loss.data_ptr(), parts.data_ptr(), L.ptr(dl),
                                           bad.data_ptr(), ks, nk, ranks, blk, L.cur_stream()), "head_cross_entropy_kd")
    return loss, dl


def check_distill_settings(temperature, alpha, label_smoothing):
    if not float(temperature) > 0.0:
        raise ValueError("temperature must be > 0, got %r" % (temperature,))
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha must lie in [0, 1], got %r" % (alpha,))
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError("label_smoothing must lie in [0, 1], got %r" % (label_smoothing,))


class _KDFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, a, b, lam, label_smoothing, weight, teacher, temperature, alpha, ignore_index, bad, parts):
        loss, dl = kd_cross_entropy(logits.detach().float().contiguous(), a, b, lam, label_smoothing, weight, teacher, temperature, alpha,
                                    ignore_index, bad=bad, parts=parts, need_grad=ctx.needs_input_grad[0])
        ctx.dl, ctx.dtype = dl, logits.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        return ((ctx.dl * grad_output).to(ctx.dtype),) + (None,) * 11


class DistillCrossEntropyLoss(nn.Module):
    """Cross-entropy with class weights, label smoothing and a knowledge-distillation term (Hinton et al. 2015):
    ``(1 - alpha) hard + alpha kd`` with ``hard = F.cross_entropy(logits, y, weight=weight, label_smoothing=label_smoothing)`` (over
    class indices, or per row ``lam CE(a) + (1 - lam) CE(b)`` over a ``mixing.MixedTarget``, normalised by the labels' weights) and
    ``kd = T^2 F.kl_div(log_softmax(logits / T), softmax(teacher / T), reduction='batchmean')`` (include/mnas.h "distillation
    cross-entropy").  ``forward(logits, target)``: ``target`` a :class:`DistillTarget`; a bare class vector or ``MixedTarget`` means
    no teacher, and the loss is the hard term alone.  ``alpha=0`` with a ``weight`` is class-weighted cross-entropy on its own.
    ``weight``: a registered buffer (it moves with ``.to()`` / ``.cuda()``) or None.  ``last_parts``: a device tensor ``(hard, kd)``
    of the last call, for logging without a host read (None after a call without weight and teacher, which is the soft-target loss
    itself and has no parts).  Differentiable with respect to the logits only.  ``Trainer`` recognises this
    class and runs the whole step without autograd (head.NativeHead.cross_entropy_kd).  No CPU path."""

    def __init__(self, temperature: float = 1.0, alpha: float = 0.5, label_smoothing: float = 0.0, weight=None, ignore_index: int = -100):
        super().__init__()
        check_distill_settings(temperature, alpha, label_smoothing)
        self.temperature, self.alpha, self.label_smoothing = float(temperature), float(alpha), float(label_smoothing)
        self.ignore_index = int(ignore_index)
        self.register_buffer("weight", check_class_weight(weight))
        self._bad = {}                   # device -> int32 flag raised by a refused label or weight
        self._parts = {}                 # device -> fp32 (2,): (hard, kd) of the last call
        self.last_parts = None

    def buffers_for(self, device):
        """(refused-target flag, parts) on ``device``; ``last_parts`` then names that device's parts tensor"""
        bad = self._bad.get(device)
        if bad is None:
            bad = self._bad[device] = torch.zeros(1, dtype=torch.int32, device=device)
            self._parts[device] = torch.zeros(2, dtype=torch.float32, device=device)
        self.last_parts = self._parts[device]
        return bad, self.last_parts

    def class_weight(self, logits):
        """the weight buffer checked against the logits' class count and device, or None"""
        w = self.weight
        if w is None:
            return None
        if w.numel() != logits.shape[1]:
            raise ValueError("weight has %d entries, the logits %d classes" % (w.numel(), logits.shape[1]))
        _on_device("weight", w, logits.device)
        return w

    def forward(self, logits, target):
        _on_device("logits", logits)
        if logits.dim() != 2:
            raise ValueError("logits must be (N, C), got %s" % (tuple(logits.shape),))
        if isinstance(target, DistillTarget):
            target.check_device(logits.device)
        a, b, lam, teacher = split_distill_target(target)
        _on_device("target", a, logits.device)
        bad, parts = self.buffers_for(logits.device)
        if teacher is None and self.weight is None:           # the soft-target loss itself, bit for bit a MixCrossEntropyLoss
            self.last_parts = None
            return _SoftCEFn.apply(logits, a, b, lam, self.label_smoothing, self.ignore_index, bad)
        return _KDFn.apply(logits, a, b, lam, self.label_smoothing, self.class_weight(logits), teacher, self.temperature, self.alpha,
                           self.ignore_index, bad, parts)

    def check_targets(self):
        """Host check of the device-side flag a label outside [0, C) or a weight outside [0, 1] raises (the loss is NaN from that
        call on).  Synchronises; resets the flag."""
        for bad in self._bad.values():
            if int(bad.item()) != 0:
                bad.zero_()
                raise ValueError("DistillCrossEntropyLoss: a label was outside [0, num_classes) and not ignore_index, or a weight outside [0, 1]")

    def extra_repr(self):
        return "temperature=%g, alpha=%g, label_smoothing=%g, weight=%s, ignore_index=%d" % (
            self.temperature, self.alpha, self.label_smoothing, "None" if self.weight is None else "(%d,)" % self.weight.numel(),
            self.ignore_index)


class HardDice(nn.Module):
    def __init__(self, threshold=0.5, deduct_intersection=False):
        super().__init__()
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError("threshold must lie inside (0, 1): the prediction is outputs > logit(threshold), got %r" % (threshold,))
        self.threshold = threshold
        self.deduct_intersection = deduct_intersection

    def forward(self, outputs, targets):
        _on_device("outputs", outputs)
        _on_device("targets", targets, outputs.device)
        if outputs.dim() != 2 or targets.shape != outputs.shape:
            raise ValueError("outputs and targets must both be (N, C), got %s and %s" % (tuple(outputs.shape), tuple(targets.shape)))
        lib = L.load()
        N, Cn = outputs.shape
        z = outputs.detach().float().contiguous()
        t = targets.detach().float().contiguous()
        th = float(self.threshold)
        out = torch.empty((), dtype=torch.float32, device=z.device)
        scratch = _scratch(lib, N, z.device)
        L.check(lib.mnas_mlabel_hard_dice(z.data_ptr(), t.data_ptr(), N, Cn, math.log(th / (1.0 - th)), 1 if self.deduct_intersection else 0,
                                          scratch.data_ptr(), out.data_ptr(), L.cur_stream()), "mlabel_hard_dice")
        return out
