"""Random Erasing (Zhong et al. 2017) on the uint8 batches the stem reads, on the GPU (csrc/mnas_imge.hip; the bytes are stated in
include/mnas.h "Random Erasing").  The boxes are overwritten in place: the batch stays ``(N, 3, H, W)`` uint8 on the device, the
kernel writes the erased area and reads nothing, and the labels are untouched, so ``Trainer.step`` takes the batch as it is.

    ra, erase, mix = DeviceRandAugment(2, 9), DeviceRandomErasing(0.25, mode="pixel"), DeviceMix(cutmix_alpha=1.0)
    for batch, target in loader:
        x = erase(ra(tf(batch.to("cuda", non_blocking=True))))       # between RandAugment and the mix
        loss = trainer.step(*mix(x, target.cuda(non_blocking=True)))

``mode="pixel"`` is the recipe's per-pixel N(0, 1) noise in normalised space, carried to byte space: the device draws 12 bits per
pixel from a counter-based Philox4x32-10 stream (csrc/mnas_rng.h) and looks them up in :func:`erase_table`, the 4096 quantiles of
N(mean_c, std_c) rounded to bytes.  A byte cannot hold the noise's tails -- with the ImageNet constants about 3 % of the quantiles
clamp at 0 or 255 -- and the 12-bit table has 4096 levels where the float recipe has a continuum; what it buys is bytes that are a
pure function of (seed, box position, n, c, y, x), which tests/erase_ref.py restates in numpy.

The draws are made on the host with the ``random`` module, as mixing.py makes its own; the descriptors of all box positions go up in
ONE pinned, non-blocking copy and nothing is read back.  No CPU path: tensors must live on the MI355X."""
from __future__ import annotations

import functools
import math
import random
from collections import namedtuple
from statistics import NormalDist
from typing import List, Tuple

import torch

from . import _lib as L

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# one box of one image: mode (L.IMGE_CONST or L.IMGE_NOISE), box (y0, x0, y1, x1), fill (the three bytes CONST writes)
EraseBox = namedtuple("EraseBox", "mode box fill")


@functools.lru_cache(maxsize=None)
def _table(mean: Tuple[float, ...], std: Tuple[float, ...]) -> bytes:
    inv = [NormalDist().inv_cdf((i + 0.5) / L.IMGE_TABLE) for i in range(L.IMGE_TABLE)]
    out = bytearray()
    for m, s in zip(mean, std):
        out += bytes(min(max(int(math.floor(255.0 * (m + s * q) + 0.5)), 0), 255) for q in inv)
    return bytes(out)


def erase_table(mean=IMAGENET_MEAN, std=IMAGENET_STD) -> bytes:
    """The 3 x 4096 bytes the NOISE mode indexes: ``T_c[i] = clamp(floor(255 (mean_c + std_c Phi^-1((i + 0.5) / 4096)) + 0.5), 0, 255)``
    with ``statistics.NormalDist().inv_cdf`` -- N(0, 1) in normalised space seen from byte space, by quantile.  Entries whose value
    falls outside a byte clamp (ImageNet constants: 72 + 51, 87 + 32 and 149 + 17 of 4096 at 0 + 255 per channel)."""
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or not all(math.isfinite(v) for v in mean + std) or not all(v >= 0.0 for v in std):
        raise ValueError("mean and std must be three finite numbers each, std >= 0")
    return _table(mean, std)


_device_tables = {}


def _device_table(mean, std, device: torch.device) -> torch.Tensor:
    """:func:`erase_table` on ``device``, uploaded once per (mean, std, device)"""
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), device.type, device.index)
    t = _device_tables.get(key)
    if t is None:
        t = _device_tables[key] = torch.frombuffer(bytearray(erase_table(mean, std)), dtype=torch.uint8).to(device)
    return t


class DeviceRandomErasing:
    """Random Erasing of an ``(N, 3, H, W)`` uint8 CUDA batch, in place.

    ``prob``: the chance that an image is erased at all.  ``min_area`` / ``max_area``: the share of the image ALL boxes of an image
    aim at together.  ``min_aspect`` / ``max_aspect``: the box's height / width, log-uniform (``max_aspect=None``: ``1 / min_aspect``).
    ``mode``: ``"const"`` fills with ``value`` (three bytes), ``"rand"`` with one colour per box taken from :func:`erase_table`,
    ``"pixel"`` with per-pixel noise.  ``min_count`` / ``max_count``: boxes per erased image (``max_count=None``: ``min_count``).
    ``mean`` / ``std``: the normalisation the model applies, which shapes the table.

    Draw order of :meth:`describe` (module-level ``random``), per image in order:

    1. ``random.random()`` -- erased iff it is ``< prob``; otherwise the image's draws end here (no box);
    2. the box count: ``min_count``, or ``random.randint(min_count, max_count)`` when they differ;
    3. per box, up to 10 attempts of
       a. ``area = random.uniform(min_area, max_area) * h * w / count``;
       b. ``aspect = exp(random.uniform(log(min_aspect), log(max_aspect)))``;
          ``bh = int(round(sqrt(area * aspect)))``, ``bw = int(round(sqrt(area / aspect)))``;
       c. accepted when ``bw < w and bh < h``: ``top = random.randint(0, h - bh)``, ``left = random.randint(0, w - bw)``, then for
          ``"rand"`` three ``random.getrandbits(12)``, channel c's colour being ``table[c][bits]``; the box's attempts end.
       A box no attempt fits is dropped, and so is an accepted box without a pixel (``bh == 0`` or ``bw == 0``), after its draws.

    After the last image one ``random.getrandbits(64)`` is the call's noise seed (drawn whatever the mode).  Boxes of one image may
    overlap; the later one wins."""

    MODES = ("const", "rand", "pixel")

    def __init__(self, prob: float = 0.25, min_area: float = 0.02, max_area: float = 1.0 / 3.0, min_aspect: float = 0.3,
                 max_aspect=None, mode: str = "pixel", value=(0, 0, 0), min_count: int = 1, max_count=None,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD):
        if not 0.0 <= float(prob) <= 1.0:
            raise ValueError("prob must lie in [0, 1]")
        if not 0.0 < float(min_area) <= float(max_area):
            raise ValueError("0 < min_area <= max_area")
        max_aspect = 1.0 / float(min_aspect) if max_aspect is None and float(min_aspect) > 0.0 else max_aspect
        if max_aspect is None or not 0.0 < float(min_aspect) <= float(max_aspect):
            raise ValueError("0 < min_aspect <= max_aspect")
        if mode not in self.MODES:
            raise ValueError("mode must be one of %s" % (self.MODES,))
        value = tuple(int(v) for v in value)
        if len(value) != 3 or not all(0 <= v <= 255 for v in value):
            raise ValueError("value must be three bytes")
        max_count = min_count if max_count is None else max_count
        if not 1 <= int(min_count) <= int(max_count):
            raise ValueError("1 <= min_count <= max_count")
        self.prob, self.min_area, self.max_area = float(prob), float(min_area), float(max_area)
        self.log_aspect = (math.log(float(min_aspect)), math.log(float(max_aspect)))
        self.mode, self.value, self.min_count, self.max_count = mode, value, int(min_count), int(max_count)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.table = erase_table(self.mean, self.std)

    def _box(self, h: int, w: int, count: int):
        """step 3 for one box -> EraseBox or None"""
        for _ in range(10):
            area = random.uniform(self.min_area, self.max_area) * h * w / count
            aspect = math.exp(random.uniform(*self.log_aspect))
            bh, bw = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if bw < w and bh < h:
                top = random.randint(0, h - bh)
                left = random.randint(0, w - bw)
                fill = self.value
                if self.mode == "rand":
                    fill = tuple(self.table[c * L.IMGE_TABLE + random.getrandbits(12)] for c in range(3))
                if bh == 0 or bw == 0:
                    return None
                return EraseBox(L.IMGE_NOISE if self.mode == "pixel" else L.IMGE_CONST, (top, left, top + bh, left + bw), fill)
        return None

    def describe(self, n: int, h: int, w: int):
        """-> ``(draws, seed)``: ``draws[k]`` is the list of image k's :class:`EraseBox` records (empty: not erased), position by
        position; ``seed`` the 64 bits the noise is keyed with.  The order is documented on the class."""
        n, h, w = int(n), int(h), int(w)
        draws: List[List[EraseBox]] = []
        for _ in range(n):
            boxes: List[EraseBox] = []
            if random.random() < self.prob:
                count = self.min_count if self.min_count == self.max_count else random.randint(self.min_count, self.max_count)
                for _ in range(count):
                    box = self._box(h, w, count)
                    if box is not None:
                        boxes.append(box)
            draws.append(boxes)
        return draws, random.getrandbits(64)

    @staticmethod
    def items(draws, position: int):
        """ctypes array of MnasImgErase (include/mnas.h) for box position ``position`` of ``draws``: an image with fewer boxes is NONE"""
        arr = (L.MnasImgErase * max(1, len(draws)))()
        for k, boxes in enumerate(draws):
            if position < len(boxes):
                b = boxes[position]
                arr[k] = L.MnasImgErase(int(b.mode), *(int(v) for v in b.box), (L.C.c_uint8 * 3)(*(int(v) for v in b.fill)), 0,
                                        (L.C.c_int32 * 2)(0, 0))
        return arr

    def apply(self, x: torch.Tensor, draws, seed: int) -> torch.Tensor:
        """Run explicit draws (:meth:`describe`'s records) on ``x``, a contiguous ``(N, 3, H, W)`` uint8 batch on an MI355X, IN PLACE;
        returns ``x``.  Every position's descriptors are checked by ``mnas_img_erase_check`` before anything is launched; they go up
        in one pinned non-blocking copy; one launch per box position that has a box."""
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("DeviceRandomErasing runs on the MI355X only (no CPU path): x must be a CUDA tensor")
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError("x must be a contiguous (N, 3, H, W) uint8 batch, got %s %s" % (tuple(x.shape), x.dtype))
        n, _, h, w = x.shape
        if len(draws) != n:
            raise ValueError("one list of boxes per image")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed must fit 64 bits")
        lib = L.load()
        positions = max((len(b) for b in draws), default=0)
        arrs = [self.items(draws, p) for p in range(positions)]
        for arr in arrs:
            rc = lib.mnas_img_erase_check(arr, n, h, w)
            if rc != 0:
                raise ValueError("erase descriptors refused by mnas_img_erase_check (code %d)" % rc)
        if n == 0 or positions == 0:
            return x
        dev = x.device
        noise = any(b.mode == L.IMGE_NOISE for boxes in draws for b in boxes)
        host = torch.empty(32 * n * positions, dtype=torch.uint8).pin_memory()
        for p, arr in enumerate(arrs):
            host[32 * n * p:32 * n * (p + 1)].copy_(torch.frombuffer(bytearray(arr), dtype=torch.uint8)[:32 * n])
        with torch.cuda.device(dev):
            table = _device_table(self.mean, self.std, dev) if noise else None
            buf = host.to(dev, non_blocking=True)
            for p in range(positions):
                L.check(lib.mnas_img_erase(buf.data_ptr() + 32 * n * p, n, h, w, x.data_ptr(), L.ptr(table), seed, p, L.cur_stream()),
                        "mnas_img_erase")
        return x

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise RuntimeError("DeviceRandomErasing runs on the MI355X only (no CPU path): x must be a CUDA tensor")
        if x.dim() != 4:
            raise ValueError("x must be a contiguous (N, 3, H, W) uint8 batch, got %s" % (tuple(x.shape),))
        return self.apply(x, *self.describe(x.shape[0], x.shape[2], x.shape[3]))
