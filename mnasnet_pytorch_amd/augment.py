"""Augmentation policies on the uint8 batches the stem reads, on the GPU (csrc/mnas_imga.hip; the ops are defined, each as the
Pillow call it equals byte for byte, in include/mnas.h "augmentation-policy ops").  The batch stays ``(N, 3, H, W)`` uint8 on the
device between ``DevicePipeline`` and the network:

    tf = DevicePipeline.from_reference(5)
    ra = DeviceRandAugment(num_ops=2, magnitude=9)
    for batch, target in loader:
        x = ra(tf(batch.to("cuda", non_blocking=True)))          # (N, 3, H, W) uint8
        loss = trainer.step(x, target.cuda(non_blocking=True))

The draws are made on the host with the ``random`` module, as transforms.py and mixing.py make theirs; the descriptors go up in ONE
pinned, non-blocking copy and nothing is read back.  No CPU path: tensors must live on the MI355X."""
from __future__ import annotations

import ctypes
import math
import random
from collections import namedtuple
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

# one op of one image: the policy's name for it and the sign drawn (0 / 1; informational), then what the kernel reads: op
# (L.IMGA_*), factor (the enhancers' blend factor) and args (AFFINE: the 16.16 fixed-point matrix a0..a5; POSTERIZE: bits;
# SOLARIZE: threshold)
AugOp = namedtuple("AugOp", "name sign op factor args")

RANDAUG_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
               "Posterize", "Solarize", "AutoContrast", "Equalize")
_SIGNED = frozenset(RANDAUG_OPS[1:10])
_ENHANCERS = {"Brightness": L.IMGA_BRIGHTNESS, "Color": L.IMGA_COLOR, "Contrast": L.IMGA_CONTRAST, "Sharpness": L.IMGA_SHARPNESS}
_STATS_OPS = (L.IMGA_CONTRAST, L.IMGA_AUTOCONTRAST, L.IMGA_EQUALIZE)
_ITEM_WORDS = ctypes.sizeof(L.MnasImgAug) // 4


def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def affine_args(matrix: Sequence[float]) -> Tuple[int, ...]:
    """Pillow's ``(a, b, c, d, e, f)`` of ``Image.transform(size, AFFINE, ...)`` -> the six 16.16 fixed-point values of an AFFINE op
    (include/mnas.h).  With ``b == d == 0`` Pillow leaves fixed point, and only unit scale with whole-pixel translations gives the
    same bytes there: anything else of that form raises."""
    a, b, c, d, e, f = (float(v) for v in matrix)
    if b == 0.0 and d == 0.0 and not (a == 1.0 and e == 1.0 and c == int(c) and f == int(f)):
        raise ValueError("an affine matrix with b == d == 0 must be a whole-pixel translation at unit scale, got %r" % (tuple(matrix),))
    return (_fix(a), _fix(b), _fix(c + a * 0.5 + b * 0.5), _fix(d), _fix(e), _fix(f + d * 0.5 + e * 0.5))


def rotate_matrix(degrees: float, h: int, w: int) -> Tuple[float, ...]:
    """the matrix ``PIL.Image.rotate(degrees)`` builds for an h x w image: cos / sin rounded to 15 decimals, about ``(w/2, h/2)``"""
    angle = -math.radians(degrees)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def aug_items(rows):
    """ctypes array of MnasImgAug (include/mnas.h) from one op list per image; an op is an :class:`AugOp` or ``(op, factor, args)``"""
    n = len(rows)
    words = np.zeros((max(1, n), _ITEM_WORDS), dtype=np.int32)
    factors = words.view(np.float32)
    for i, ops in enumerate(rows):
        if len(ops) > L.IMGA_MAX_OPS:
            raise ValueError("at most %d ops per image, got %d" % (L.IMGA_MAX_OPS, len(ops)))
        words[i, 0] = len(ops)
        for k, o in enumerate(ops):
            op, factor, args = o[-3:]
            if len(args) > 6:
                raise ValueError("an op takes at most six integer arguments")
            words[i, 1 + k] = int(op)
            factors[i, 5 + k] = float(factor)
            words[i, 9 + 6 * k:9 + 6 * k + len(args)] = [int(v) for v in args]
    return (L.MnasImgAug * max(1, n)).from_buffer(words)


def aug_plan(arr, n):
    """(longest chain, stage mask of the statistics ops) of the first n items, chains right-aligned as mnas_img_aug runs them"""
    if n == 0:
        return 0, 0
    words = np.frombuffer(arr, dtype=np.int32).reshape(-1, _ITEM_WORDS)[:n]
    nops = np.clip(words[:, 0], 0, L.IMGA_MAX_OPS)
    max_ops = int(nops.max())
    stages = 0
    for k in range(L.IMGA_MAX_OPS):
        has = (nops > k) & np.isin(words[:, 1 + k], _STATS_OPS)
        for length in np.unique(nops[has]):
            stages |= 1 << (max_ops - int(length) + k)
    return max_ops, stages


def aug_apply(x: torch.Tensor, items, fill=(0, 0, 0), out=None) -> torch.Tensor:
    """Run op chains on a contiguous ``(N, 3, H, W)`` uint8 CUDA batch ``x`` -> ``out`` (new unless given; never ``x`` itself).
    ``items``: one op list per image (:func:`aug_items`' format) or a ctypes array of MnasImgAug.  ``fill``: the RGB bytes AFFINE
    puts where the source falls outside the image.  Raises ``ValueError`` for whatever ``mnas_img_aug_check`` refuses, before any
    launch; descriptors go up in one pinned copy; launched on the current stream."""
    lib = L.load()
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("aug_apply runs on the MI355X only (no CPU path): x must be a CUDA tensor")
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise ValueError("x must be a contiguous (N, 3, H, W) uint8 batch, got %s %s" % (tuple(x.shape), x.dtype))
    n, _, h, w = x.shape
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError("fill must be three bytes (r, g, b)")
    arr = items if isinstance(items, ctypes.Array) else aug_items(items)
    if len(arr) < n or (not isinstance(items, ctypes.Array) and len(items) != n):
        raise ValueError("one descriptor per image")
    if out is None:
        out = torch.empty_like(x)
    elif (not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != torch.uint8 or not out.is_contiguous()
          or out.device != x.device):
        raise ValueError("out must be a contiguous uint8 %s tensor on x's device" % (tuple(x.shape),))
    if out.data_ptr() == x.data_ptr() and n > 0:
        raise ValueError("aug_apply runs out of place: out must not be x")
    rc = lib.mnas_img_aug_check(arr, n, h, w)
    if rc != 0:
        raise ValueError("augmentation descriptors refused by mnas_img_aug_check (code %d)" % rc)
    if n == 0:
        return out
    max_ops, stages = aug_plan(arr, n)
    dev = x.device
    host = torch.frombuffer(bytearray(arr), dtype=torch.uint8).pin_memory()
    with torch.cuda.device(dev):
        dev_items = host.to(dev, non_blocking=True)
        nbytes = lib.mnas_img_aug_workspace_bytes(n, h, w, max_ops, int(stages != 0))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes > 0 else None
        L.check(lib.mnas_img_aug(dev_items.data_ptr(), n, h, w, max_ops, stages, fill[0] | fill[1] << 8 | fill[2] << 16,
                                 x.data_ptr(), out.data_ptr(), L.ptr(ws), L.cur_stream()), "mnas_img_aug")
    return out


class DeviceRandAugment:
    """RandAugment (Cubuk et al. 2020) on an ``(N, 3, H, W)`` uint8 CUDA batch: per image ``num_ops`` ops drawn from 14, all at
    magnitude ``magnitude`` of ``num_magnitude_bins`` linear steps, each byte for byte the Pillow call that defines it.

    Draw order of :meth:`describe` (module-level ``random``), image after image and within an image op position after op position:

    1. ``random.randrange(14)`` picks from ``RANDAUG_OPS``: Identity, ShearX, ShearY, TranslateX, TranslateY, Rotate, Brightness,
       Color, Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize;
    2. for the signed ops (the shears, translations, Rotate and the four enhancers), ``random.randrange(2) == 1`` negates the magnitude.

    The magnitude table is torchvision's RandAugment table, step ``i = magnitude`` of ``bins`` linear steps from the first value to
    the second: shear 0 .. 0.3; translation 0 .. 150/331 of the width (X) or height (Y), truncated with ``int()``; rotation
    0 .. 30 degrees; enhancer factor ``1 +- (0 .. 0.9)``; posterize bits ``8 - round(4 i / (bins - 1))``; solarize threshold
    255 .. 0 (rounded up to the integer with the same effect).  Matrices, in Pillow's ``(a, b, c, d, e, f)``: ShearX ``(1, m, 0, 0,
    1, 0)``, ShearY ``(1, 0, 0, m, 1, 0)``, TranslateX ``(1, 0, t, 0, 1, 0)``, TranslateY ``(1, 0, 0, 0, 1, t)``, Rotate the matrix
    ``PIL.Image.rotate(degrees)`` builds; nearest-neighbour, ``fill`` outside.  A zero magnitude becomes Identity.

    The draw order and these matrices are this package's own (as ``transforms.get_params`` is): the op set and the magnitudes follow
    torchvision, but a seed does not reproduce torchvision's draws."""

    def __init__(self, num_ops: int = 2, magnitude: int = 9, num_magnitude_bins: int = 31, fill=(0, 0, 0)):
        if not 0 <= int(num_ops) <= L.IMGA_MAX_OPS:
            raise ValueError("num_ops must lie in [0, %d]" % L.IMGA_MAX_OPS)
        if int(num_magnitude_bins) < 2 or not 0 <= int(magnitude) < int(num_magnitude_bins):
            raise ValueError("magnitude must index one of num_magnitude_bins >= 2 steps")
        fill = tuple(int(v) for v in fill)
        if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
            raise ValueError("fill must be three bytes (r, g, b)")
        self.num_ops, self.magnitude, self.num_magnitude_bins, self.fill = int(num_ops), int(magnitude), int(num_magnitude_bins), fill

    def op(self, name: str, sign: int, h: int, w: int) -> AugOp:
        """the magnitude table: the named op at this policy's magnitude on an h x w image, negated when ``sign`` is 1"""
        step = self.magnitude / float(self.num_magnitude_bins - 1)
        s = -1.0 if sign else 1.0
        ident = AugOp(name, sign, L.IMGA_IDENTITY, 0.0, ())
        if name == "Identity":
            return ident
        if name in ("ShearX", "ShearY"):
            m = s * 0.3 * step
            if m == 0.0:
                return ident
            return AugOp(name, sign, L.IMGA_AFFINE, 0.0, affine_args((1, m, 0, 0, 1, 0) if name == "ShearX" else (1, 0, 0, m, 1, 0)))
        if name in ("TranslateX", "TranslateY"):
            t = int(s * (150.0 / 331.0 * (w if name == "TranslateX" else h)) * step)
            if t == 0:
                return ident
            return AugOp(name, sign, L.IMGA_AFFINE, 0.0,
                         affine_args((1, 0, t, 0, 1, 0) if name == "TranslateX" else (1, 0, 0, 0, 1, t)))
        if name == "Rotate":
            deg = s * 30.0 * step
            if deg == 0.0:
                return ident
            return AugOp(name, sign, L.IMGA_AFFINE, 0.0, affine_args(rotate_matrix(deg, h, w)))
        if name in _ENHANCERS:
            m = s * 0.9 * step
            if m == 0.0:
                return ident
            return AugOp(name, sign, _ENHANCERS[name], 1.0 + m, ())
        if name == "Posterize":
            return AugOp(name, sign, L.IMGA_POSTERIZE, 0.0, (8 - int(round(4.0 * self.magnitude / (self.num_magnitude_bins - 1))),))
        if name == "Solarize":
            return AugOp(name, sign, L.IMGA_SOLARIZE, 0.0, (int(math.ceil(255.0 - 255.0 * step)),))
        if name == "AutoContrast":
            return AugOp(name, sign, L.IMGA_AUTOCONTRAST, 0.0, ())
        if name == "Equalize":
            return AugOp(name, sign, L.IMGA_EQUALIZE, 0.0, ())
        raise ValueError("unknown op %r" % (name,))

    def describe(self, n: int, size: Tuple[int, int]) -> List[List[AugOp]]:
        """one list of ``num_ops`` :class:`AugOp` per image of an ``n x 3 x H x W`` batch, ``size = (H, W)``, in the order documented
        on the class"""
        h, w = int(size[0]), int(size[1])
        rows = []
        for _ in range(int(n)):
            ops = []
            for _ in range(self.num_ops):
                name = RANDAUG_OPS[random.randrange(14)]
                sign = random.randrange(2) if name in _SIGNED else 0
                ops.append(self.op(name, sign, h, w))
            rows.append(ops)
        return rows

    def __call__(self, x: torch.Tensor, out=None) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("DeviceRandAugment runs on the MI355X only (no CPU path): x must be a CUDA tensor")
        if x.dim() != 4:
            raise ValueError("x must be a contiguous (N, 3, H, W) uint8 batch, got %s" % (tuple(x.shape),))
        return aug_apply(x, self.describe(x.shape[0], (x.shape[2], x.shape[3])), self.fill, out=out)
