"""The reference's input pipeline on the GPU (datasets.py ``preprocess_img``): crop, PIL-bilinear resize and flips of decoded
uint8 images (``Resize``, ``CenterCrop``, ``RandomResizedCropRect``, ``RandomHorizontalFlip``) and the photometric ops of
preprocessing type 3 (``ColorJitter``, ``RandomGrayscale``), batched into the NCHW uint8 tensor the stem reads with
``model.normalize_on_device()``.  Every output image equals, byte for byte, what Pillow makes of it:

    flips(window(PIL.Image.crop(img, box).resize((rw, rh), Image.BILINEAR)))          (csrc/mnas_imgx.hip, ``apply``)
    ImageEnhance.{Brightness,Contrast,Color}.enhance(f), adjust_hue, convert('L')   (csrc/mnas_imgc.hip, ``color_apply``)

(tests/img_xform_ref.py and tests/img_color_ref.py restate both in numpy and are held to Pillow).  JPEG decoding stays on the
CPU.

    loader = DataLoader(dataset, batch_size=B, sampler=ClusterRandomSampler(dataset, B), collate_fn=collate_decoded,
                        num_workers=8, pin_memory=True)
    tf = DevicePipeline.from_reference(3)                     # any of types 0-6; sizes from the dataset (ImageBatch.target_size)
    model.normalize_on_device()
    for batch, target in loader:
        x = tf(batch.to("cuda", non_blocking=True))          # (B, 3, H, W) uint8 on the current stream
        loss = trainer.step(x, target.cuda(non_blocking=True))

Random draws (crop boxes, flips, jitter factors and their order, grayscale) happen on the host with Python's module-level
``random`` in the order torchvision 0.2.x draws them, like ``sampler.py``: ``random.seed(s)`` reproduces the descriptors.
"""
from __future__ import annotations

import ctypes
import math
import random
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

__all__ = ["ImageBatch", "collate_decoded", "DeviceTransform", "get_params", "color_apply", "DeviceColorJitter",
           "DeviceRandomGrayscale", "DevicePipeline", "Type3Draw"]


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
            raise ValueError("preprocessing_type 3 (ColorJitter, RandomGrayscale, two resamples) is not a single transform: "
                             "use DevicePipeline.from_reference(3)")
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


# ---- photometric ops (preprocessing type 3) ----
_JITTER_OPS = (L.IMGC_BRIGHTNESS, L.IMGC_CONTRAST, L.IMGC_SATURATION, L.IMGC_HUE)


def hue_shift(hue_factor: float) -> int:
    """torchvision 0.2.x ``adjust_hue`` adds ``np.uint8(hue_factor * 255)`` to H; numpy 1.x truncated toward zero and wrapped
    (numpy 2 raises for a negative value, so this never calls np.uint8 on it): ``int(hue_factor * 255) mod 256``."""
    return int(hue_factor * 255) % 256


def color_items(desc):
    """ctypes array of MnasImgColor (include/mnas.h) for ``desc``: one ``[(op, value), ...]`` per image, applied in order.
    ``value`` is the blend factor of BRIGHTNESS / CONTRAST / SATURATION, the torchvision hue factor (in [-0.5, 0.5]) of HUE,
    ignored for GRAY; at most one HUE per image."""
    arr = (L.MnasImgColor * max(1, len(desc)))()
    for k, ops in enumerate(desc):
        if len(ops) > L.IMGC_MAX_OPS:
            raise ValueError("at most %d ops per image" % L.IMGC_MAX_OPS)
        it = arr[k]
        it.nops = len(ops)
        hues = [v for op, v in ops if op == L.IMGC_HUE]
        if len(hues) > 1:
            raise ValueError("one hue op per image")
        if hues and not -0.5 <= hues[0] <= 0.5:
            raise ValueError("hue factor %r is not in [-0.5, 0.5]" % (hues[0],))
        it.hue_shift = hue_shift(hues[0]) if hues else 0
        for j, (op, v) in enumerate(ops):
            it.op[j] = int(op)
            it.factor[j] = 0.0 if op in (L.IMGC_HUE, L.IMGC_GRAY) else float(v)
    return arr


def _batch_shape(layout, n, h, w):
    return (n, 3, h, w) if layout == L.IMGC_NCHW else (n, h, w, 3)


def color_apply(x: torch.Tensor, items, in_layout: int, out_layout: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Run photometric descriptors on a contiguous uint8 CUDA batch ``x``: ``(N, 3, H, W)`` (``IMGC_NCHW``) or ``(N, H, W, 3)``
    (``IMGC_NHWC``) -> ``out`` in ``out_layout`` (new unless given; ``out is x`` runs in place, same layout only).  ``items``:
    ``color_items``' format (one op list per image) or a ctypes array of MnasImgColor.  Checked by ``mnas_img_color_check``,
    uploaded in one pinned copy, launched on the current stream."""
    lib = L.load()
    if x.device.type != "cuda" or x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
        raise ValueError("color_apply needs a contiguous 4-D uint8 tensor on an MI355X device")
    if in_layout not in (L.IMGC_NCHW, L.IMGC_NHWC) or out_layout not in (L.IMGC_NCHW, L.IMGC_NHWC):
        raise ValueError("layouts are IMGC_NCHW or IMGC_NHWC")
    n = x.shape[0]
    h, w = (x.shape[2], x.shape[3]) if in_layout == L.IMGC_NCHW else (x.shape[1], x.shape[2])
    if tuple(x.shape) != _batch_shape(in_layout, n, h, w):
        raise ValueError("x has shape %s, not a 3-channel batch in layout %d" % (tuple(x.shape), in_layout))
    arr = items if isinstance(items, ctypes.Array) else color_items(items)
    if len(arr) < n or (not isinstance(items, ctypes.Array) and len(items) != n):
        raise ValueError("one descriptor per image")
    if out is None:
        out = torch.empty(_batch_shape(out_layout, n, h, w), dtype=torch.uint8, device=x.device)
    elif (tuple(out.shape) != _batch_shape(out_layout, n, h, w) or out.dtype != torch.uint8 or not out.is_contiguous()
          or out.device != x.device):
        raise ValueError("out must be a contiguous uint8 %s tensor on x's device" % (_batch_shape(out_layout, n, h, w),))
    if out.data_ptr() == x.data_ptr() and in_layout != out_layout:
        raise ValueError("in place only with equal layouts")
    rc = lib.mnas_img_color_check(arr, n, h, w)
    if rc != 0:
        raise ValueError("image color descriptors refused by mnas_img_color_check (code %d)" % rc)
    if n == 0:
        return out
    contrast = any(arr[k].op[j] == L.IMGC_CONTRAST for k in range(n) for j in range(arr[k].nops))
    dev = x.device
    host = torch.frombuffer(bytearray(arr), dtype=torch.uint8).pin_memory()
    with torch.cuda.device(dev):
        dev_items = host.to(dev, non_blocking=True)
        ws = torch.empty(lib.mnas_img_color_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev) if contrast else None
        L.check(lib.mnas_img_color(dev_items.data_ptr(), n, h, w, in_layout, x.data_ptr(), out_layout, out.data_ptr(),
                                   L.ptr(ws), L.cur_stream()), "mnas_img_color")
    return out


class DeviceColorJitter:
    """torchvision 0.2.x ``ColorJitter(brightness, contrast, saturation, hue)`` on an ``(N, 3, H, W)`` uint8 CUDA batch, byte for
    byte Pillow's result per image.  Draws per image, one image after another, as 0.2.x ``get_params`` does (module-level
    ``random``): ``uniform(max(0, 1 - b), 1 + b)`` for brightness, contrast, saturation, then ``uniform(-h, h)`` for hue, each
    only if its parameter is > 0, then ``random.shuffle`` of the ops drawn."""

    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0):
        for v in (brightness, contrast, saturation):
            if not v >= 0:
                raise ValueError("brightness, contrast and saturation must be >= 0")
        if not 0 <= hue <= 0.5:
            raise ValueError("hue must be in [0, 0.5]")
        self.brightness, self.contrast, self.saturation, self.hue = (float(v) for v in (brightness, contrast, saturation, hue))

    def draw(self) -> List[Tuple[int, float]]:
        """one image's ``[(op, factor)]`` in the order they apply"""
        ops = []
        for op, v in zip(_JITTER_OPS[:3], (self.brightness, self.contrast, self.saturation)):
            if v > 0:
                ops.append((op, random.uniform(max(0, 1 - v), 1 + v)))
        if self.hue > 0:
            ops.append((L.IMGC_HUE, random.uniform(-self.hue, self.hue)))
        random.shuffle(ops)
        return ops

    def describe(self, n: int) -> List[List[Tuple[int, float]]]:
        return [self.draw() for _ in range(n)]

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return color_apply(x, self.describe(x.shape[0]), L.IMGC_NCHW, L.IMGC_NCHW)


class DeviceRandomGrayscale:
    """torchvision 0.2.x ``RandomGrayscale(p)`` on an ``(N, 3, H, W)`` uint8 CUDA batch: one ``random.random() < p`` per image
    (drawn whatever p), ``convert('L')`` replicated to three channels."""

    def __init__(self, p: float = 0.1):
        self.p = float(p)

    def describe(self, n: int) -> List[bool]:
        return [random.random() < self.p for _ in range(n)]

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return color_apply(x, [[(L.IMGC_GRAY, 0.0)] if g else [] for g in self.describe(x.shape[0])], L.IMGC_NCHW, L.IMGC_NCHW)


# one image's draws of preprocessing type 3: applied (RandomApply), jitter ([(op, factor)] in order, None unless applied),
# box ((top, left, h, w) of the RandomResizedCropRect in the final_size image, None unless applied), flags (IMGX_HFLIP |
# IMGX_VFLIP), gray (RandomGrayscale)
Type3Draw = namedtuple("Type3Draw", "applied jitter box flags gray")


class DevicePipeline:
    """``preprocess_img(preprocessing_type)`` of the reference (datasets.py) for any type 0-6 on a GPU ``ImageBatch`` ->
    ``(N, 3, Ho, Wo)`` uint8.  Types other than 3 are ``DeviceTransform.from_reference`` (same bytes, same draws).  Type 3 is

        Resize(final_size), RandomApply([ColorJitter(.1, .1, .1, .1), RandomResizedCropRect(final_size, (0.7, 1.0),
        (0.7, 1.2))], p=prob), RandomHorizontalFlip(prob), RandomVerticalFlip(prob), RandomGrayscale(prob)

    with torchvision 0.2.x's draws (restated from that release: torchvision is not installed here): RandomApply's
    ``prob < random.random()`` skips the pair; ColorJitter's ``get_params`` then the crop's; then one ``random.random() < prob``
    per flip and for grayscale, drawn even when prob is 0.  It runs as four launches: resize to final_size (NCHW scratch);
    the jitter ops NCHW -> NHWC scratch (a plain transpose for images not jittered); crop box (the whole image when not
    jittered: a same-size bilinear resample is the identity, as in Pillow) and flips back to final_size; grey in place."""

    def __init__(self, preprocessing_type: int, final_size=None, fixed_size=(224, 224), prob: float = 0.2):
        self.preprocessing_type = int(preprocessing_type)
        self.final_size = None if final_size is None else (int(final_size[0]), int(final_size[1]))
        self.prob = float(prob)
        if self.preprocessing_type == 3:
            self.transform = None
            self.jitter = DeviceColorJitter(0.1, 0.1, 0.1, 0.1)
            self.scale, self.ratio = (0.7, 1.0), (0.7, 1.2)
        else:
            self.transform = DeviceTransform.from_reference(self.preprocessing_type, final_size, fixed_size)

    @classmethod
    def from_reference(cls, preprocessing_type: int, final_size=None, fixed_size=(224, 224), prob: float = 0.2):
        return cls(preprocessing_type, final_size, fixed_size, prob)

    def out_size(self, target_size=None) -> Tuple[int, int]:
        if self.transform is not None:
            return self.transform.out_size(target_size)
        size = self.final_size if self.final_size is not None else target_size
        if size is None:
            raise ValueError("no output size: pass final_size= or have the dataset report its target size")
        return int(size[0]), int(size[1])

    def describe(self, shapes, target_size=None):
        """((Ho, Wo), per-image draws in the reference's order): ``DeviceTransform.describe`` tuples for types other than 3,
        ``Type3Draw`` records for type 3"""
        if self.transform is not None:
            return self.transform.describe(shapes, target_size)
        fh, fw = self.out_size(target_size)
        out = []
        for _ in shapes:
            applied = not self.prob < random.random()
            jitter = box = None
            if applied:
                jitter = tuple(self.jitter.draw())
                box = get_params(fh, fw, self.scale, self.ratio)
            flags = 0
            if random.random() < self.prob:
                flags |= L.IMGX_HFLIP
            if random.random() < self.prob:
                flags |= L.IMGX_VFLIP
            out.append(Type3Draw(applied, jitter, box, flags, random.random() < self.prob))
        return (fh, fw), out

    def __call__(self, batch: ImageBatch, size=None) -> torch.Tensor:
        if self.transform is not None:
            return self.transform(batch, size)
        (fh, fw), draws = self.describe(batch.shapes, size if size is not None else batch.target_size)
        return run_type3(batch, draws, (fh, fw))


def run_type3(batch: ImageBatch, draws, final_size) -> torch.Tensor:
    """Run explicit type-3 draws (``DevicePipeline.describe``'s ``Type3Draw`` records) on a GPU ``ImageBatch``."""
    fh, fw = int(final_size[0]), int(final_size[1])
    n = len(batch)
    if len(draws) != n:
        raise ValueError("one draw per image")
    resized = apply(batch, [(0, 0, h, w, fh, fw, 0, 0, 0) for h, w, _ in batch.shapes], (fh, fw))
    if n == 0:
        return resized
    nbytes = n * fh * fw * 3
    scratch = torch.empty((nbytes + 15) & ~15, dtype=torch.uint8, device=batch.device)      # ImageBatch: 16-byte multiple
    jittered = scratch[:nbytes].view(n, fh, fw, 3)
    color_apply(resized, [list(d.jitter) if d.applied else [] for d in draws], L.IMGC_NCHW, L.IMGC_NHWC, out=jittered)
    src = ImageBatch(scratch, [(fh, fw, 3)] * n, [k * fh * fw * 3 for k in range(n)])
    out = apply(src, [tuple(d.box if d.applied else (0, 0, fh, fw)) + (fh, fw, 0, 0, d.flags) for d in draws], (fh, fw))
    if any(d.gray for d in draws):
        color_apply(out, [[(L.IMGC_GRAY, 0.0)] if d.gray else [] for d in draws], L.IMGC_NCHW, L.IMGC_NCHW, out=out)
    return out
