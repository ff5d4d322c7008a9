"""Batch mixing -- Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) -- on the uint8 batches the stem reads, on the GPU
(csrc/mnas_imgm.hip; the arithmetic is stated in include/mnas.h "batch mixing").  The mixed batch stays ``(N, 3, H, W)`` uint8 on
the device; the two labels and the weight of every row travel as a :class:`MixedTarget`, which ``losses.MixCrossEntropyLoss`` and
``Trainer.step`` take in place of the class vector.  A multi-label batch travels as a :class:`MixedLabels` (the unmixed ``(N, C)``
label matrix, the partner row indices and the weights), which ``losses.MultiLabelLoss`` takes in place of the label matrix.

    mix = DeviceMix(mixup_alpha=0.2, cutmix_alpha=1.0)
    trainer = Trainer(model, criterion=MixCrossEntropyLoss(label_smoothing=0.1))
    for batch, target in loader:
        x = tf(batch.to("cuda", non_blocking=True))              # transforms.DevicePipeline: (N, 3, H, W) uint8
        x, mixed = mix(x, target.cuda(non_blocking=True))
        loss = trainer.step(x, mixed)

The draws are made on the host with the ``random`` module, as transforms.py makes its own; the descriptors, the partner indices and
the weights go up in ONE pinned, non-blocking copy and nothing is read back.  No CPU path: tensors must live on the MI355X."""
from __future__ import annotations

import math
import random
from collections import namedtuple
from typing import List

import torch

from . import _lib as L

# one image's draw: mode (L.IMGM_*), partner (index into the batch), w16 (MIXUP: weight of the image itself, 0..65536), box
# ((y0, x0, y1, x1), CUTMIX: the region taken from the partner), lam (the weight of the image's own label that the pixels really got)
MixDraw = namedtuple("MixDraw", "mode partner w16 box lam")


class MixedTarget:
    """The labels of a mixed batch: row n is ``lam[n]`` of class ``a[n]`` and ``1 - lam[n]`` of class ``b[n]``.  ``a``, ``b``: int64
    ``(N,)``; ``lam``: fp32 ``(N,)`` in [0, 1]; all three on one MI355X device."""

    def __init__(self, a: torch.Tensor, b: torch.Tensor, lam: torch.Tensor):
        for name, t, dt in (("a", a, torch.int64), ("b", b, torch.int64), ("lam", lam, torch.float32)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
                raise TypeError("MixedTarget.%s must be a 1-D %s tensor" % (name, dt))
        if not (a.shape == b.shape == lam.shape):
            raise ValueError("a, b and lam must have the same length, got %d, %d, %d" % (a.numel(), b.numel(), lam.numel()))
        if not (a.device == b.device == lam.device):
            raise RuntimeError("a, b and lam must be on one device, got %s, %s, %s" % (a.device, b.device, lam.device))
        self.a, self.b, self.lam = a.contiguous(), b.contiguous(), lam.contiguous()

    @property
    def device(self):
        return self.a.device

    @property
    def shape(self):
        return self.a.shape

    def __len__(self):
        return self.a.shape[0]

    def to(self, device, non_blocking: bool = False) -> "MixedTarget":
        return MixedTarget(*(t.to(device, non_blocking=non_blocking) for t in (self.a, self.b, self.lam)))

    def check_device(self, device):
        """the kernels take raw device pointers: everything on ``device``, an MI355X"""
        if self.device.type != "cuda":
            raise RuntimeError("a MixedTarget must be on the MI355X (no CPU path)")
        if self.device != torch.device(device):
            raise RuntimeError("the MixedTarget is on %s, the logits on %s (the kernels take raw device pointers)" % (self.device, device))

    def dominant(self) -> torch.Tensor:
        """the label that carries the larger weight, ``a`` when ``lam >= 0.5``: what the accuracy meters count a row against"""
        return torch.where(self.lam >= 0.5, self.a, self.b)

    def __repr__(self):
        return "MixedTarget(N=%d, device=%s)" % (len(self), self.device)


class MixedLabels:
    """The labels of a mixed multi-label batch: row n is ``lam[n]`` of the label row ``labels[n]`` and ``1 - lam[n]`` of
    ``labels[partner[n]]``.  ``labels``: fp32 ``(N, C)`` (soft values allowed), the UNMIXED label matrix; ``partner``: int64
    ``(N,)`` row indices; ``lam``: fp32 ``(N,)`` in [0, 1]; all three on one MI355X device.  ``losses.MultiLabelLoss`` forms the
    mixed row on load (include/mnas.h "multi-label loss"); nothing is gathered or materialised."""

    def __init__(self, labels: torch.Tensor, partner: torch.Tensor, lam: torch.Tensor):
        for name, t, dt, nd in (("labels", labels, torch.float32, 2), ("partner", partner, torch.int64, 1), ("lam", lam, torch.float32, 1)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != nd:
                raise TypeError("MixedLabels.%s must be a %d-D %s tensor" % (name, nd, dt))
        if not (labels.shape[0] == partner.shape[0] == lam.shape[0]):
            raise ValueError("labels, partner and lam must have the same number of rows, got %d, %d, %d"
                             % (labels.shape[0], partner.numel(), lam.numel()))
        if not (labels.device == partner.device == lam.device):
            raise RuntimeError("labels, partner and lam must be on one device, got %s, %s, %s" % (labels.device, partner.device, lam.device))
        self.labels, self.partner, self.lam = labels.detach().contiguous(), partner.contiguous(), lam.contiguous()

    @property
    def device(self):
        return self.labels.device

    @property
    def shape(self):
        return self.labels.shape

    def __len__(self):
        return self.labels.shape[0]

    def to(self, device, non_blocking: bool = False) -> "MixedLabels":
        return MixedLabels(*(t.to(device, non_blocking=non_blocking) for t in (self.labels, self.partner, self.lam)))

    def check_device(self, device):
        """the kernels take raw device pointers: everything on ``device``, an MI355X"""
        if self.device.type != "cuda":
            raise RuntimeError("a MixedLabels must be on the MI355X (no CPU path)")
        if self.device != torch.device(device):
            raise RuntimeError("the MixedLabels is on %s, the logits on %s (the kernels take raw device pointers)" % (self.device, device))

    def dominant(self) -> torch.Tensor:
        """``(N, C)``: the label row of the image that carries the larger weight, row n when ``lam >= 0.5``: what the multi-label
        meters count a row against"""
        return torch.where((self.lam >= 0.5).unsqueeze(1), self.labels, self.labels.index_select(0, self.partner))

    def dense(self) -> torch.Tensor:
        """``(N, C)``: the materialised ``lam Y + (1 - lam) Y[partner]``, for a criterion that takes a soft label matrix"""
        lam = self.lam.unsqueeze(1)
        return lam * self.labels + (1.0 - lam) * self.labels.index_select(0, self.partner)

    def __repr__(self):
        return "MixedLabels(N=%d, C=%d, device=%s)" % (len(self), self.labels.shape[1], self.device)


def cutmix_box(h: int, w: int, lam: float, cy: int, cx: int):
    """The CutMix paper's box for weight ``lam`` around the centre ``(cy, cx)``: sides ``int(h r), int(w r)`` with
    ``r = sqrt(1 - lam)``, edges clipped to the image.  -> ``((y0, x0, y1, x1), lam_eff)`` with ``lam_eff = 1 - area / (h w)``, the
    weight the pixels really got."""
    r = math.sqrt(1.0 - lam)
    ch, cw = int(h * r), int(w * r)
    y0, y1 = min(max(cy - ch // 2, 0), h), min(max(cy + ch // 2, 0), h)
    x0, x1 = min(max(cx - cw // 2, 0), w), min(max(cx + cw // 2, 0), w)
    return (y0, x0, y1, x1), 1.0 - (y1 - y0) * (x1 - x0) / float(h * w)


class DeviceMix:
    """Mixup and / or CutMix of an ``(N, 3, H, W)`` uint8 CUDA batch with a permutation of itself.

    ``mixup_alpha`` / ``cutmix_alpha``: the Beta(alpha, alpha) the weight is drawn from; 0 turns that mode off (both 0: nothing is
    mixed).  ``prob``: the chance that a draw mixes at all.  ``switch_prob``: with both modes on, the chance of CutMix.
    ``per_sample``: one draw per image instead of one for the whole batch.

    Draw order of :meth:`describe` (module-level ``random``), for ``n > 0``:

    1. ``random.sample(range(n), n)``: image k's partner is the k-th entry (an image may draw itself);
    2. then one draw for the whole batch, or with ``per_sample`` one per image in order, each made of
       a. ``random.random()`` -- mixed iff it is ``< prob`` and an alpha is on; otherwise the draw ends here (mode NONE, weight 1);
       b. with both alphas on, ``random.random() < switch_prob`` chooses CutMix;
       c. ``random.betavariate(alpha, alpha)`` with the chosen mode's alpha: the weight ``lam``;
       d. CutMix only: ``random.randrange(h)``, ``random.randrange(w)``: the centre of :func:`cutmix_box`.

    The weight that reaches the loss is the one the pixels really got: ``w16 / 65536`` with ``w16 = round(lam * 65536)`` for Mixup,
    ``1 - box_area / (h w)`` for CutMix."""

    def __init__(self, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0, switch_prob: float = 0.5,
                 per_sample: bool = False):
        if not (float(mixup_alpha) >= 0.0 and float(cutmix_alpha) >= 0.0):
            raise ValueError("mixup_alpha and cutmix_alpha must be >= 0 (0: off)")
        if not (0.0 <= float(prob) <= 1.0 and 0.0 <= float(switch_prob) <= 1.0):
            raise ValueError("prob and switch_prob must lie in [0, 1]")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.per_sample = float(prob), float(switch_prob), bool(per_sample)

    def _draw(self, h: int, w: int):
        """steps a-d -> (mode, w16, box, lam)"""
        none = (L.IMGM_NONE, 65536, (0, 0, 0, 0), 1.0)
        on = self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0
        if not (random.random() < self.prob and on):
            return none
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = random.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0.0
        if cut:
            lam = random.betavariate(self.cutmix_alpha, self.cutmix_alpha)
            cy, cx = random.randrange(h), random.randrange(w)
            box, lam_eff = cutmix_box(h, w, lam, cy, cx)
            return (L.IMGM_CUTMIX, 65536, box, lam_eff)
        lam = random.betavariate(self.mixup_alpha, self.mixup_alpha)
        w16 = int(round(lam * 65536.0))
        return (L.IMGM_MIXUP, w16, (0, 0, 0, 0), w16 / 65536.0)

    def describe(self, n: int, h: int, w: int) -> List[MixDraw]:
        """one :class:`MixDraw` per image, in the order documented on the class"""
        n, h, w = int(n), int(h), int(w)
        if n == 0:
            return []
        partners = random.sample(range(n), n)
        if self.per_sample:
            draws = [self._draw(h, w) for _ in range(n)]
        else:
            draws = [self._draw(h, w)] * n
        return [MixDraw(mode, k if mode == L.IMGM_NONE else partners[k], w16, box, lam)
                for k, (mode, w16, box, lam) in enumerate(draws)]

    @staticmethod
    def items(draws):
        """ctypes array of MnasImgMix (include/mnas.h) for ``draws``"""
        arr = (L.MnasImgMix * max(1, len(draws)))()
        for k, d in enumerate(draws):
            arr[k] = L.MnasImgMix(int(d.mode), int(d.partner), int(d.w16), *(int(v) for v in d.box), 0)
        return arr

    @staticmethod
    def apply(x: torch.Tensor, target: torch.Tensor, draws):
        """Run explicit draws (:meth:`describe`'s records) -> ``(mixed uint8 batch, MixedTarget)``.  ``x``: contiguous ``(N, 3, H, W)``
        uint8 on an MI355X, left as it is (the pass is out of place); ``target``: int64 ``(N,)`` on the same device.  Checked by
        ``mnas_img_mix_check``; descriptors, partner indices and weights go up in one pinned non-blocking copy.  A floating
        ``(N, C)`` label matrix as ``target`` (the multi-label branch) -> ``(mixed uint8 batch, MixedLabels(target, partner
        indices, weights))``: the same bytes from the same draws, no gather and no launch more."""
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("DeviceMix runs on the MI355X only (no CPU path): x must be a CUDA tensor")
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError("x must be a contiguous (N, 3, H, W) uint8 batch, got %s %s" % (tuple(x.shape), x.dtype))
        n, _, h, w = x.shape
        matrix = isinstance(target, torch.Tensor) and target.is_floating_point() and target.dim() == 2 and target.shape[0] == n
        if not matrix and (not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or target.shape != (n,)):
            raise ValueError("target must be int64 of shape (N,), or a floating (N, C) label matrix")
        if target.device != x.device:
            raise RuntimeError("target is on %s, x on %s (the kernels take raw device pointers)" % (target.device, x.device))
        if len(draws) != n:
            raise ValueError("one draw per image")
        lib = L.load()
        arr = DeviceMix.items(draws)
        rc = lib.mnas_img_mix_check(arr, n, h, w)
        if rc != 0:
            raise ValueError("mix descriptors refused by mnas_img_mix_check (code %d)" % rc)
        out = torch.empty_like(x)
        dev = x.device
        if n == 0:
            z = torch.empty(0, dtype=torch.int64, device=dev)
            if matrix:
                return out, MixedLabels(target.float(), z, torch.empty(0, dtype=torch.float32, device=dev))
            return out, MixedTarget(z, z.clone(), torch.empty(0, dtype=torch.float32, device=dev))
        # one host buffer: [n MnasImgMix (32 bytes each) | n int64 partner indices | n fp32 weights]
        host = torch.empty(44 * n, dtype=torch.uint8).pin_memory()
        host[:32 * n].copy_(torch.frombuffer(bytearray(arr), dtype=torch.uint8)[:32 * n])
        host[32 * n:40 * n].view(torch.int64).copy_(torch.tensor([int(d.partner) for d in draws], dtype=torch.int64))
        host[40 * n:].view(torch.float32).copy_(torch.tensor([float(d.lam) for d in draws], dtype=torch.float32))
        with torch.cuda.device(dev):
            buf = host.to(dev, non_blocking=True)
            L.check(lib.mnas_img_mix(buf.data_ptr(), n, h, w, x.data_ptr(), out.data_ptr(), L.cur_stream()), "mnas_img_mix")
            if matrix:                   # the loss reads the partner's label row through the index: nothing is gathered here
                return out, MixedLabels(target.float(), buf[32 * n:40 * n].view(torch.int64), buf[40 * n:].view(torch.float32))
            target = target.contiguous()
            partner = target.index_select(0, buf[32 * n:40 * n].view(torch.int64))
        return out, MixedTarget(target, partner, buf[40 * n:].view(torch.float32))

    def __call__(self, x: torch.Tensor, target: torch.Tensor):
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("DeviceMix runs on the MI355X only (no CPU path): x must be a CUDA tensor")
        if x.dim() != 4:
            raise ValueError("x must be a contiguous (N, 3, H, W) uint8 batch, got %s" % (tuple(x.shape),))
        return self.apply(x, target, self.describe(x.shape[0], x.shape[2], x.shape[3]))
