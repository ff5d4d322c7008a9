"""The geometric half of the reference's input pipeline on the GPU: crop, PIL-bilinear resize and flips of decoded uint8 images
(datasets.py ``preprocess_img``: ``Resize``, ``CenterCrop``, ``RandomResizedCropRect``, ``RandomHorizontalFlip``), batched into the
NCHW uint8 tensor the stem reads with ``model.normalize_on_device()``.  Every output image equals, byte for byte,

    flips(window(PIL.Image.crop(img, box).resize((rw, rh), Image.BILINEAR)))

(csrc/mnas_imgx.hip; tests/img_xform_ref.py restates it in numpy and is held to Pillow).  JPEG decoding and the photometric
augmentations (type 3: ``ColorJitter``, ``RandomGrayscale``) stay on the CPU.

    loader = DataLoader(dataset, batch_size=B, sampler=ClusterRandomSampler(dataset, B), collate_fn=collate_decoded,
                        num_workers=8, pin_memory=True)
    tf = DeviceTransform.from_reference(4)                   # sizes from the dataset (ImageBatch.target_size)
    model.normalize_on_device()
    for batch, target in loader:
        x = tf(batch.to("cuda", non_blocking=True))          # (B, 3, H, W) uint8 on the current stream
        loss = trainer.step(x, target.cuda(non_blocking=True))

Random draws (crop boxes, flips) happen on the host with Python's module-level ``random``, like ``sampler.py``: ``random.seed(s)``
reproduces the descriptors.
"""
from __future__ import annotations

import math
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

__all__ = ["ImageBatch", "collate_decoded", "DeviceTransform", "get_params"]


def _as_hwc(img) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(img))
    if a.dtype != np.uint8:
        raise TypeError("decoded images must be uint8, got %s" % a.dtype)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("decoded images must be HxW or HxWxC with C in (1, 3, 4), got shape %s" % (a.shape,))
    return a


class ImageBatch:
    """N decoded HWC uint8 images back to back in one uint8 buffer (padded to a multiple of 16 bytes), with their
    ``shapes`` ``(h, w, c)`` and byte ``offsets``.  ``target_size`` is the batch's output size if the dataset reported one
    (``collate_decoded``).  Built on the host the buffer is pinned when a GPU is present (not inside DataLoader workers:
    ``DataLoader(pin_memory=True)`` pins it through ``pin_memory()``)."""

    def __init__(self, data: torch.Tensor, shapes, offsets, target_size=None):
        if data.dtype != torch.uint8 or data.dim() != 1 or data.numel() % 16 or data.numel() < 16:
            raise ValueError("ImageBatch.data must be a 1-D uint8 tensor of a positive multiple of 16 bytes")
        self.data = data
        self.shapes: List[Tuple[int, int, int]] = [tuple(int(v) for v in s) for s in shapes]
        self.offsets: List[int] = [int(o) for o in offsets]
        self.target_size = None if target_size is None else tuple(int(v) for v in target_size)
        if len(self.shapes) != len(self.offsets):
            raise ValueError("one offset per image")

    @classmethod
    def from_arrays(cls, images: Sequence, pin: Optional[bool] = None, target_size=None) -> "ImageBatch":
        arrays = [_as_hwc(a) for a in images]
        offsets, total = [], 0
        for a in arrays:
            offsets.append(total)
            total += a.nbytes
        if pin is None:
            pin = torch.cuda.is_available() and torch.utils.data.get_worker_info() is None
        data = torch.empty(max(16, (total + 15) & ~15), dtype=torch.uint8, pin_memory=bool(pin))
        buf = data.numpy()
        for a, o in zip(arrays, offsets):
            buf[o:o + a.nbytes] = a.reshape(-1)
        buf[total:] = 0
        return cls(data, [a.shape for a in arrays], offsets, target_size)

    def __len__(self) -> int:
        return len(self.shapes)

    @property
    def device(self) -> torch.device:
        return self.data.device

    def to(self, device, non_blocking: bool = False) -> "ImageBatch":
        return ImageBatch(self.data.to(device, non_blocking=non_blocking), self.shapes, self.offsets, self.target_size)

    def pin_memory(self) -> "ImageBatch":
        return ImageBatch(self.data.pin_memory(), self.shapes, self.offsets, self.target_size)

    def image(self, i: int) -> np.ndarray:
        """image i as an HWC numpy view (host batches only)"""
        h, w, c = self.shapes[i]
        o = self.offsets[i]
        return self.data.numpy()[o:o + h * w * c].reshape(h, w, c)


def collate_decoded(samples):
    """``DataLoader`` ``collate_fn`` for a dataset returning ``(HWC uint8 array, target)`` or ``(array, target, target_size)``:
    images of any sizes go into one ``ImageBatch`` (the default collate cannot stack them), targets through the default
    collate.  A ``target_size`` (the reference's ``final_size``, one per resolution cluster) must agree across the batch and
    becomes ``ImageBatch.target_size``.  Returns ``(ImageBatch, targets)``."""
    sizes = {tuple(int(v) for v in s[2]) for s in samples if len(s) > 2}
    if len(sizes) > 1:
        raise ValueError("one target size per batch (use ClusterRandomSampler): got %s" % sorted(sizes))
    batch = ImageBatch.from_arrays([s[0] for s in samples], target_size=sizes.pop() if sizes else None)
    return batch, torch.utils.data.default_collate([s[1] for s in samples])


def get_params(h: int, w: int, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.)) -> Tuple[int, int, int, int]:
    """``RandomResizedCrop.get_params`` of the torchvision the reference was written against (0.2.x; torchvision is not
    installed here, so the draw order is restated from that release, not pinned against it): ten attempts of
    ``uniform(scale) * area`` and ``uniform(ratio)``, sides ``round(sqrt(.))``, a coin flip that swaps them, ``randint``
    placement; then the centred square.  One guard added: a side that rounds to 0 is rejected like one that does not fit
    (0.2.x would hand PIL an empty crop).  Module-level ``random``.  Returns (top, left, box_h, box_w)."""
    area = w * h
    for _ in range(10):
        target_area = random.uniform(*scale) * area
        aspect_ratio = random.uniform(*ratio)
        cw = int(round(math.sqrt(target_area * aspect_ratio)))
        ch = int(round(math.sqrt(target_area / aspect_ratio)))
        if random.random() < 0.5:
            cw, ch = ch, cw
        if 0 < cw <= w and 0 < ch <= h:
            return random.randint(0, h - ch), random.randint(0, w - cw), ch, cw
    s = min(w, h)
    return (h - s) // 2, (w - s) // 2, s, s


def _shorter_side(h: int, w: int, s: int) -> Tuple[int, int]:
    """torchvision ``Resize(int)``: the shorter side becomes s, the longer int(s * long / short); unchanged if already s"""
    if (w <= h and w == s) or (h <= w and h == s):
        return h, w
    if w < h:
        return int(s * h / w), s
    return s, int(s * w / h)


class DeviceTransform:
    """One call turns an ``ImageBatch`` on the GPU into the ``(N, 3, Ho, Wo)`` uint8 batch (current torch stream).

    mode ``"resize"``: whole image -> ``size`` (h, w).  ``"shorter_side_center_crop"``: shorter side -> ``size`` (an int), then
    the centred ``crop`` (h, w) window.  ``"random_resized_crop"``: box from ``get_params(scale, ratio)`` -> ``size``.
    ``hflip`` / ``vflip``: flip probabilities, drawn per image after its box (``random.random() < p``).  ``size=None`` (resize,
    random_resized_crop): the batch's ``target_size``.  Descriptors are drawn on the host, validated by
    ``mnas_img_xform_check`` and uploaded in one small copy before the launch."""

    MODES = ("resize", "shorter_side_center_crop", "random_resized_crop")

    def __init__(self, mode: str, size=None, crop=None, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), hflip: float = 0.0,
                 vflip: float = 0.0):
        if mode not in self.MODES:
            raise ValueError("mode must be one of %s" % (self.MODES,))
        if mode == "shorter_side_center_crop" and (not isinstance(size, int) or crop is None):
            raise ValueError("shorter_side_center_crop needs an int size and a (h, w) crop")
        self.mode = mode
        self.size = size if size is None or isinstance(size, int) else (int(size[0]), int(size[1]))
        self.crop = None if crop is None else (int(crop[0]), int(crop[1]))
        self.scale, self.ratio = tuple(scale), tuple(ratio)
        self.hflip, self.vflip = float(hflip), float(vflip)

    @classmethod
    def from_reference(cls, preprocessing_type: int, final_size=None, fixed_size=(224, 224)) -> "DeviceTransform":
        """The geometry of ``ImnetDataset.preprocess_img(preprocessing_type)`` (datasets.py).  ``final_size`` is the reference's
        ``[int(s * size_ratio) for s in target_size]``; None = per batch from ``ImageBatch.target_size``."""
        fixed = (int(fixed_size[0]), int(fixed_size[1]))
        if preprocessing_type == 0:
            return cls("resize", fixed)
        if preprocessing_type == 1:
            return cls("shorter_side_center_crop", fixed[0], crop=fixed)
        if preprocessing_type == 2:
            return cls("resize", final_size)
        if preprocessing_type == 4:
            return cls("random_resized_crop", final_size, hflip=0.5)
        if preprocessing_type == 5:
            return cls("random_resized_crop", fixed, hflip=0.5)
        if preprocessing_type == 6:
            return cls("random_resized_crop", fixed, scale=(0.7, 1.0), ratio=(0.7, 1.2), hflip=0.5)
        if preprocessing_type == 3:
            raise ValueError("preprocessing_type 3 (ColorJitter, RandomGrayscale, two resamples) is not supported on the device")
        raise ValueError("This augmentation is not supported")

    def out_size(self, target_size=None) -> Tuple[int, int]:
        if self.mode == "shorter_side_center_crop":
            return self.crop
        size = self.size if self.size is not None else target_size
        if size is None:
            raise ValueError("no output size: pass size= to DeviceTransform or have the dataset report its target size")
        return int(size[0]), int(size[1])

    def describe(self, shapes, target_size=None) -> Tuple[Tuple[int, int], List[Tuple[int, ...]]]:
        """((Ho, Wo), [(box_top, box_left, box_h, box_w, rh, rw, win_top, win_left, flags) per image]) for images of
        ``shapes`` (h, w[, c]); draws from the module-level ``random`` in image order."""
        ho, wo = self.out_size(target_size)
        out = []
        for s in shapes:
            h, w = int(s[0]), int(s[1])
            if self.mode == "resize":
                box, rs, win = (0, 0, h, w), (ho, wo), (0, 0)
            elif self.mode == "shorter_side_center_crop":
                rs = _shorter_side(h, w, self.size)
                win = (int(round((rs[0] - ho) / 2.)), int(round((rs[1] - wo) / 2.)))
                if win[0] < 0 or win[1] < 0 or win[0] + ho > rs[0] or win[1] + wo > rs[1]:
                    raise ValueError("center crop %s larger than the resized image %s" % ((ho, wo), rs))
                box = (0, 0, h, w)
            else:
                box, rs, win = get_params(h, w, self.scale, self.ratio), (ho, wo), (0, 0)
            flags = 0
            if self.hflip > 0 and random.random() < self.hflip:
                flags |= L.IMGX_HFLIP
            if self.vflip > 0 and random.random() < self.vflip:
                flags |= L.IMGX_VFLIP
            out.append(tuple(box) + tuple(rs) + tuple(win) + (flags,))
        return (ho, wo), out

    @staticmethod
    def descriptors(batch: ImageBatch, desc):
        """ctypes array of MnasImgXform (include/mnas.h) for ``describe``'s tuples; images back to back (stride w * c)"""
        arr = (L.MnasImgXform * max(1, len(desc)))()
        for k, (d, (h, w, c), off) in enumerate(zip(desc, batch.shapes, batch.offsets)):
            arr[k] = L.MnasImgXform(off, h, w, c, w * c, *d, 0)
        return arr

    def __call__(self, batch: ImageBatch, size=None) -> torch.Tensor:
        (ho, wo), desc = self.describe(batch.shapes, size if size is not None else batch.target_size)
        return apply(batch, desc, (ho, wo))


def apply(batch: ImageBatch, desc, out_size) -> torch.Tensor:
    """Run explicit descriptors (``DeviceTransform.describe`` format) on a GPU ``ImageBatch``: (N, 3, Ho, Wo) uint8."""
    lib = L.load()
    dev = batch.device
    if dev.type != "cuda":
        raise RuntimeError("the ImageBatch must be on an MI355X device: batch.to('cuda', non_blocking=True)")
    ho, wo = int(out_size[0]), int(out_size[1])
    n = len(batch)
    if len(desc) != n:
        raise ValueError("one descriptor per image")
    arr = DeviceTransform.descriptors(batch, desc)
    src_bytes = batch.data.numel()
    rc = lib.mnas_img_xform_check(arr, n, ho, wo, src_bytes)
    if rc != 0:
        raise ValueError("image transform descriptors refused by mnas_img_xform_check (code %d)" % rc)
    out = torch.empty((n, 3, ho, wo), dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    host = torch.frombuffer(bytearray(arr), dtype=torch.uint8).pin_memory()
    with torch.cuda.device(dev):
        items = host.to(dev, non_blocking=True)
        L.check(lib.mnas_img_xform(items.data_ptr(), n, ho, wo, batch.data.data_ptr(), src_bytes, out.data_ptr(),
                                   L.cur_stream()), "mnas_img_xform")
    return out
