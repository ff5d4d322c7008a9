"""numpy restatement of the image batch transform (csrc/mnas_imgx.hip, include/mnas.h MnasImgXform): Pillow's 8-bit bilinear
resampler (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the horizontal pass first, then the vertical one), the crop in
front of it, the window and the flips behind it.  Vectorised over rows, columns and channels; every tap loop runs in tap order
in fp64 exactly as Pillow does, so the coefficients are bit-identical (tests/test_img_xform_cpu.py holds this file to Pillow).

    out = flips(window(PIL.Image.crop(src, box).resize((rw, rh), Image.BILINEAR)))   ->  (3, Ho, Wo) uint8
"""
import math

import numpy as np

PRECISION_BITS = 22                # 32 - 8 - 2
HFLIP, VFLIP = 1, 2


def coeffs(inn, out, first=0, count=None):
    """(xmin, xmax, kk) of output indices [first, first + count) of an axis inn -> out: xmin / xmax int64 (count,),
    kk int64 (count, ksize), zero past xmax."""
    count = out - first if count is None else count
    scale = inn / out                                   # Python float: fp64, as (double)(in1 - in0) / outSize
    fs = max(scale, 1.0)
    support = fs                                        # bilinear support 1.0 * filterscale
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int) truncates toward zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), inn) - xmin
    taps = np.arange(ksize, dtype=np.int64)
    t = ((taps[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    t = np.abs(t)
    w = np.where(t < 1.0, 1.0 - t, 0.0)
    w[taps[None, :] >= xmax[:, None]] = 0.0
    ww = np.zeros(count, dtype=np.float64)
    for j in range(ksize):                              # in tap order (numpy's own sum is pairwise)
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)
    return xmin, xmax, kk


def clip8(acc):
    return np.where(acc <= 0, 0, np.where(acc >= (1 << (PRECISION_BITS + 8)), 255, acc >> PRECISION_BITS)).astype(np.uint8)


def _pass(img, out, first, count):
    """one resampling pass along axis 1 of img (rows, inn, 3) uint8 -> (rows, count, 3) uint8"""
    inn = img.shape[1]
    xmin, _, kk = coeffs(inn, out, first, count)
    acc = np.full((img.shape[0], count, img.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for j in range(kk.shape[1]):
        idx = np.minimum(xmin + j, inn - 1)              # kk is 0 past xmax
        acc += img[:, idx, :].astype(np.int64) * kk[None, :, j, None]
    return clip8(acc)


def to_rgb(img):
    """HWC (or HW) uint8 -> HW3: grey replicated (cv2.COLOR_GRAY2RGB), alpha dropped"""
    img = np.asarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    c = img.shape[2]
    if c == 1:
        return np.repeat(img, 3, axis=2)
    if c == 3:
        return img
    if c == 4:
        return img[:, :, :3]
    raise ValueError("channels must be 1, 3 or 4, got %d" % c)


def xform(img, box, rsize, window, out_size, flags=0):
    """img HWC uint8; box (top, left, h, w); rsize (rh, rw); window (top, left); out_size (Ho, Wo); flags HFLIP | VFLIP.
    -> (3, Ho, Wo) uint8.  Only the window's rows and columns are resampled (each output index depends on its own taps only)."""
    top, left, bh, bw = box
    rh, rw = rsize
    wt, wl = window
    ho, wo = out_size
    crop = to_rgb(img)[top:top + bh, left:left + bw]
    if crop.shape[:2] != (bh, bw) or wt < 0 or wl < 0 or wt + ho > rh or wl + wo > rw:
        raise ValueError("box or window outside the image")
    h = _pass(crop, rw, wl, wo)                                      # (bh, wo, 3): the horizontal pass runs first
    v = _pass(h.transpose(1, 0, 2), rh, wt, ho).transpose(1, 0, 2)   # (ho, wo, 3)
    if flags & HFLIP:
        v = v[:, ::-1]
    if flags & VFLIP:
        v = v[::-1]
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def pil_xform(img, box, rsize, window, out_size, flags=0):
    """The same through Pillow (the oracle of the restatement; needs PIL)."""
    from PIL import Image
    top, left, bh, bw = box
    rh, rw = rsize
    wt, wl = window
    ho, wo = out_size
    im = Image.fromarray(to_rgb(img), "RGB").crop((left, top, left + bw, top + bh))
    bilinear = getattr(Image, "Resampling", Image).BILINEAR
    r = np.asarray(im.resize((rw, rh), bilinear))[wt:wt + ho, wl:wl + wo]
    if flags & HFLIP:
        r = r[:, ::-1]
    if flags & VFLIP:
        r = r[::-1]
    return np.ascontiguousarray(r.transpose(2, 0, 1))
