"""Loss and top-k accuracy meters that live on the GPU: the reference's ``AverageMeter`` / ``accuracy()`` (train.py:657-700) as
it uses them after every step (train.py:447, 465-468) and every validation batch (train.py:575, 589-592), without the three
``.item()`` host reads per batch.  One ``MnasMeters`` block (include/mnas.h) in device memory is moved by HIP kernels
(csrc/mnas_head.hip) in stream order; the host copies it when it wants to print.

* :class:`DeviceMeters` -- the block: ``update`` / ``reset`` / ``read`` / ``all_reduce``.  ``Trainer(meters=...)`` feeds it from
  inside the loss kernels of the step (no extra launch); ``Trainer.validate`` runs a whole pass on it with one host sync.
* :func:`accuracy` -- drop-in for train.py:687-700 on device tensors, for scripts that keep the reference's own meters.
* :class:`MultiLabelMeters` -- the same for the multi-label branch (train.py:453-463, 577-587): loss, HardDice(0.5) and the per-sample
  macro-F1 of ``batch_metrics`` in one ``MnasMultiLabelMeters`` block (csrc/mnas_mlabel.hip), instead of a copy of the logits to
  the host and one scikit-learn call per row.

Row n is correct@k iff ``rank_n < k`` with ``rank_n = #{j: z[n,j] > z[n,t]} + #{j < t: z[n,j] == z[n,t]}``, evaluated on whatever is
handed in (logits or probabilities: softmax is monotone up to rounding).  Single-label classification only.  No CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _lib as L

_NI, _NF = L.METERS_NUM_I64, L.METERS_NUM_F64
_MI, _MF = L.MLABEL_NUM_I64, L.MLABEL_NUM_F64


class MeterValue:
    """``val`` (last update) and ``avg`` (running) of one meter -- the two numbers train.py prints per meter"""
    __slots__ = ("val", "avg")

    def __init__(self, val: float, avg: float):
        self.val, self.avg = val, avg

    def __repr__(self):
        return "MeterValue(val=%r, avg=%r)" % (self.val, self.avg)


class MetersRecord:
    """Host copy of one ``MnasMeters`` block, decoded.  ``loss.val/.avg``; ``acc[k].val/.avg`` in percent; ``correct[k]`` /
    ``last_correct[k]`` the integer counts behind them; ``loss_sum`` = ``AverageMeter.sum`` of the loss meter."""

    def __init__(self, raw: L.MnasMeters, topk: Sequence[int]):
        self.topk = tuple(topk)
        self.steps, self.samples = int(raw.steps), int(raw.samples)
        self.loss_samples, self.nonfinite_steps = int(raw.loss_samples), int(raw.nonfinite_steps)
        self.last_n, self.last_loss_n = int(raw.last_n), int(raw.last_loss_n)
        self.loss_sum, self.last_loss, self.last_loss_sum = float(raw.loss_sum), float(raw.last_loss), float(raw.last_loss_sum)
        self.correct = {k: int(raw.correct[i]) for i, k in enumerate(self.topk)}
        self.last_correct = {k: int(raw.last_correct[i]) for i, k in enumerate(self.topk)}
        # AverageMeter: avg = sum / count; val = the last value.  last_loss_sum / last_loss_n IS last_loss on one rank (an fp32
        # loss times a batch size is exact in double) and the sample-weighted mean of the ranks' last losses after all_reduce
        self.loss = MeterValue(self.last_loss_sum / self.last_loss_n if self.last_loss_n else 0.0,
                               self.loss_sum / self.loss_samples if self.loss_samples else 0.0)
        # accuracy(): correct_k * (100 / batch_size)
        self.acc: Dict[int, MeterValue] = {
            k: MeterValue(self.last_correct[k] * 100.0 / self.last_n if self.last_n else 0.0,
                          self.correct[k] * 100.0 / self.samples if self.samples else 0.0) for k in self.topk}

    def __repr__(self):
        accs = " ".join("acc%d %.4f (%.4f)" % (k, v.val, v.avg) for k, v in self.acc.items())
        return "MetersRecord(steps %d samples %d loss %.6f (%.6f) %s nonfinite_steps %d)" % (
            self.steps, self.samples, self.loss.val, self.loss.avg, accs, self.nonfinite_steps)


class DeviceMeters:
    """One ``MnasMeters`` block on ``device``.  Everything but :meth:`read` is enqueued on the current stream and returns at once."""

    def __init__(self, topk: Sequence[int] = (1, 5), device=None):
        topk = tuple(int(k) for k in topk)
        if not 1 <= len(topk) <= L.METERS_MAX_K or any(k < 1 for k in topk):
            raise ValueError("topk must hold 1..%d values of k >= 1, got %r" % (L.METERS_MAX_K, topk))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("DeviceMeters live on the MI355X (no CPU path); got device %s" % (dev,))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        assert C.sizeof(L.MnasMeters) == 8 * (_NI + _NF)
        self.topk, self.device = topk, dev
        self.lib = L.load()
        self.block = torch.zeros(_NI + _NF, dtype=torch.int64, device=dev)      # the doubles are viewed, never converted
        self._ks = (C.c_int * len(topk))(*topk)
        self._scratch = {}

    # ---- what the kernels take ------------------------------------------------------------------------------------------
    def kernel_args(self, N: int, device):
        """(ks, nk, rank_rows pointer, block pointer) for a batch of N rows on ``device`` (scratch cached per N)"""
        if torch.device(device) != self.device:
            raise RuntimeError("meters are on %s, the logits on %s (the kernels take raw device pointers)" % (self.device, device))
        rows = self._scratch.get(N)
        if rows is None:
            rows = self._scratch[N] = torch.empty(N, dtype=torch.int32, device=self.device)
        return self._ks, len(self.topk), rows.data_ptr(), self.block.data_ptr()

    def update(self, logits: torch.Tensor, target: torch.Tensor, loss: Optional[torch.Tensor] = None):
        """accuracy(logits, target, topk) and, when ``loss`` (a device scalar) is given, losses.update(loss.item(), N)."""
        if logits.dim() != 2:
            raise ValueError("logits must be (N, C), got %s" % (tuple(logits.shape),))
        N, Cn = logits.shape
        if target.dtype != torch.int64 or target.shape != (N,):
            raise ValueError("target must be int64 of shape (N,)")
        if target.device != logits.device:
            raise RuntimeError("target is on %s, logits on %s" % (target.device, logits.device))
        ks, nk, rows, blk = self.kernel_args(N, logits.device)
        logits = logits.detach().float().contiguous()
        target = target.contiguous()
        if loss is not None:
            if loss.numel() != 1 or loss.device != logits.device:
                raise ValueError("loss must be a one-element tensor on %s" % (logits.device,))
            loss = loss.detach().float().contiguous()
        L.check(self.lib.mnas_head_metrics(logits.data_ptr(), target.data_ptr(), N, Cn, ks, nk, L.ptr(loss), rows, blk,
                                           L.cur_stream()), "head_metrics")

    def reset(self):
        self.block.zero_()

    def read(self) -> MetersRecord:
        """ONE device-to-host copy of the block (which waits for everything enqueued before it)."""
        host = self.block.cpu()
        raw = L.MnasMeters()
        C.memmove(C.byref(raw), host.data_ptr(), C.sizeof(raw))
        return MetersRecord(raw, self.topk)

    def all_reduce(self, group=None):
        """Sum the block over the ranks of ``group``: the running fields become those of the whole data set; the last-update fields
        become the sum over the ranks' last steps (so ``val`` is the value over the global batch of the last step)."""
        import torch.distributed as dist
        dist.all_reduce(self.block[:_NI], op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.block[_NI:].view(torch.float64), op=dist.ReduceOp.SUM, group=group)


class MultiLabelRecord:
    """Host copy of one ``MnasMultiLabelMeters`` block, decoded.  ``loss`` / ``hdice`` / ``f1`` are ``MeterValue(val, avg)``;
    ``<meter>_sum`` / ``<meter>_n`` the ``AverageMeter.sum`` / ``.count`` behind them; ``tp`` / ``fp`` / ``fn`` the running element
    counts under the Dice rule (``last_*``: of the last update)."""

    def __init__(self, raw: L.MnasMultiLabelMeters):
        self.steps, self.samples, self.nonfinite_steps = int(raw.steps), int(raw.samples), int(raw.nonfinite_steps)
        self.tp, self.fp, self.fn = int(raw.tp), int(raw.fp), int(raw.fn)
        self.last_n, self.last_tp, self.last_fp, self.last_fn = int(raw.last_n), int(raw.last_tp), int(raw.last_fp), int(raw.last_fn)
        for name, key in (("loss", "loss"), ("hdice", "dice"), ("f1", "f1")):
            total, n = float(getattr(raw, key + "_sum")), int(getattr(raw, key + "_n"))
            last, last_sum, last_n = float(getattr(raw, "last_" + key)), float(getattr(raw, "last_%s_sum" % key)), int(getattr(raw, "last_%s_n" % key))
            # AverageMeter: avg = sum / count, val = the last value.  On one rank last * last_n reproduces last_sum and val is the
            # stored value itself; after all_reduce the three fields are sums over the ranks and val = the weighted mean of the
            # ranks' last values
            val = last if (last * last_n == last_sum or last != last) else (last_sum / last_n if last_n else 0.0)
            setattr(self, name, MeterValue(val if last_n else 0.0, total / n if n else 0.0))
            setattr(self, name + "_sum", total)
            setattr(self, name + "_n", n)
            setattr(self, "last_%s_sum" % name, last_sum)
            setattr(self, "last_%s_n" % name, last_n)

    def __repr__(self):
        return "MultiLabelRecord(steps %d samples %d loss %.6f (%.6f) hdice %.4f (%.4f) f1 %.4f (%.4f) nonfinite_steps %d)" % (
            self.steps, self.samples, self.loss.val, self.loss.avg, self.hdice.val, self.hdice.avg, self.f1.val, self.f1.avg,
            self.nonfinite_steps)


class MultiLabelMeters:
    """One ``MnasMultiLabelMeters`` block on ``device``: the loss, HardDice(0.5) and macro-F1 meters of the reference's multi-label
    branch.  Everything but :meth:`read` is enqueued on the current stream and returns at once."""

    def __init__(self, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("MultiLabelMeters live on the MI355X (no CPU path); got device %s" % (dev,))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        assert C.sizeof(L.MnasMultiLabelMeters) == 8 * (_MI + _MF)
        self.device = dev
        self.lib = L.load()
        self.block = torch.zeros(_MI + _MF, dtype=torch.int64, device=dev)      # the doubles are viewed, never converted

    def kernel_args(self, device):
        """the block's device pointer, for kernels that run on ``device``"""
        if torch.device(device) != self.device:
            raise RuntimeError("meters are on %s, the logits on %s (the kernels take raw device pointers)" % (self.device, device))
        return self.block.data_ptr()

    def update(self, logits: torch.Tensor, target: torch.Tensor, loss: Optional[torch.Tensor] = None, f1_n: Optional[int] = None):
        """hdices05.update(HardDice(0.5)(logits, target).item(), N), f1_meter.update(mean row F1, f1_n) and, when ``loss`` (a
        device scalar) is given, losses.update(loss.item(), N).  ``f1_n`` defaults to N."""
        if logits.dim() != 2:
            raise ValueError("logits must be (N, C), got %s" % (tuple(logits.shape),))
        N, Cn = logits.shape
        if target.shape != logits.shape:
            raise ValueError("target must be of shape (N, C) = %s, got %s" % (tuple(logits.shape), tuple(target.shape)))
        if target.device != logits.device:
            raise RuntimeError("target is on %s, logits on %s" % (target.device, logits.device))
        blk = self.kernel_args(logits.device)
        logits = logits.detach().float().contiguous()
        target = target.detach().float().contiguous()
        if loss is not None:
            if loss.numel() != 1 or loss.device != logits.device:
                raise ValueError("loss must be a one-element tensor on %s" % (logits.device,))
            loss = loss.detach().float().contiguous()
        scratch = torch.empty(int(self.lib.mnas_mlabel_scratch_bytes(N)), dtype=torch.uint8, device=self.device)
        L.check(self.lib.mnas_mlabel_metrics(logits.data_ptr(), target.data_ptr(), N, Cn, L.ptr(loss), scratch.data_ptr(), blk, N, N,
                                             N if f1_n is None else int(f1_n), L.cur_stream()), "mlabel_metrics")

    def reset(self):
        self.block.zero_()

    def read(self) -> MultiLabelRecord:
        """ONE device-to-host copy of the block (which waits for everything enqueued before it)."""
        host = self.block.cpu()
        raw = L.MnasMultiLabelMeters()
        C.memmove(C.byref(raw), host.data_ptr(), C.sizeof(raw))
        return MultiLabelRecord(raw)

    def all_reduce(self, group=None):
        """Sum the block over the ranks of ``group`` (see DeviceMeters.all_reduce)."""
        import torch.distributed as dist
        dist.all_reduce(self.block[:_MI], op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.block[_MI:].view(torch.float64), op=dist.ReduceOp.SUM, group=group)


def accuracy(output: torch.Tensor, target: torch.Tensor, topk: Sequence[int] = (1,)):
    """train.py:687-700 on device tensors: the precision@k in percent for every k of ``topk``, as 0-d fp32 device tensors, without a
    host sync.  (Ties: the lower class index wins; torch.topk leaves the order of equal values unspecified.)"""
    m = DeviceMeters(topk, output.device)
    m.update(output, target)
    last = m.block[_NI - L.METERS_MAX_K:_NI]               # last_correct[]
    scale = 100.0 / target.size(0)
    return [last[i].to(torch.float32).mul_(scale) for i in range(len(m.topk))]
