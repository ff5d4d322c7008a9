"""numpy restatement of the augmentation-policy ops (csrc/mnas_imga.hip, include/mnas.h MnasImgAug), of an image's op chain and
of DeviceRandAugment.describe's mapping from draws to descriptors.  Every op is the Pillow call named in include/mnas.h, restated:

    affine        Image.transform(size, AFFINE, (a, b, c, d, e, f), NEAREST, fillcolor=fill): 16.16 fixed point, FIX(v) =
                  floor(v * 65536 + 0.5); a0, a1, a3, a4 = FIX(a, b, d, e), a2 = FIX(c + a/2 + b/2), a5 = FIX(f + d/2 + e/2);
                  output (x, y) takes source ((a2 + x a0 + y a1) >> 16, (a5 + x a3 + y a4) >> 16) when that lies inside the image and
                  the fill colour otherwise.  With b == d == 0 Pillow takes another route (per-axis doubles) that gives the same
                  bytes for unit scale and whole-pixel translations: the only such matrices that ``fixed_matrix`` lets through.
    brightness / color / contrast   ImageEnhance: img_color_ref's blend with 0 / the pixel's grey / the image's rounded grey mean
    sharpness     blend(ImageFilter.SMOOTH(img), img, f); SMOOTH = (1 1 1 / 1 5 1 / 1 1 1) / 13 -> (2 s + 13) // 26 on interior
                  pixels, the outermost rows and columns copied, an image with a side < 3 unchanged
    posterize / solarize / invert   ImageOps: v & ~(2^(8 - bits) - 1); v if v < threshold else 255 - v; 255 - v
    autocontrast  ImageOps.autocontrast(img) (cutoff 0): per channel lo / hi = the first / last value present; hi <= lo: unchanged;
                  else lut[v] = clamp(int(v * scale + offset)), scale = 255.0 / (hi - lo), offset = -lo * scale in doubles
    equalize      ImageOps.equalize(img): per channel over the non-zero bins, step = (sum - last non-zero bin) // 255; one bin or
                  step == 0: unchanged; else lut[v] = min(255, (step // 2 + sum of the bins below v) // step)

tests/test_randaug_cpu.py holds every function here to the installed Pillow.  An op is a tuple ``(code, factor, args)`` with
``args`` up to six integers (AFFINE: the fixed-point matrix; POSTERIZE: bits; SOLARIZE: threshold)."""
import math
import random

import numpy as np

import img_color_ref as R

IDENTITY, AFFINE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE, INVERT, AUTOCONTRAST, EQUALIZE = range(11)  # MNAS_IMGA_*
MAX_OPS = 4
NAMES = ["Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
         "Posterize", "Solarize", "AutoContrast", "Equalize"]
SIGNED = set(NAMES[1:10])


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def fixed_matrix(m):
    """(a, b, c, d, e, f) -> (a0, a1, a2, a3, a4, a5); a matrix with b == d == 0 must be a whole-pixel translation"""
    a, b, c, d, e, f = (float(v) for v in m)
    if b == 0.0 and d == 0.0 and not (a == 1.0 and e == 1.0 and c == int(c) and f == int(f)):
        raise ValueError("with b == d == 0 only unit scale and whole-pixel translations are defined")
    return (fix(a), fix(b), fix(c + a * 0.5 + b * 0.5), fix(d), fix(e), fix(f + d * 0.5 + e * 0.5))


def rotate_matrix(deg, h, w):
    """the matrix Image.rotate(deg) hands to Image.transform (centre (w / 2, h / 2), no translation, no expand)"""
    angle = -math.radians(deg)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def affine(img, fixed, fill=(0, 0, 0)):
    h, w = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (int(v) for v in fixed)
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    xin = (a2 + x * a0 + y * a1) >> 16
    yin = (a5 + x * a3 + y * a4) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.empty_like(img)
    out[...] = np.asarray(fill, dtype=np.uint8)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def smooth(img):
    h, w = img.shape[:2]
    if h < 3 or w < 3:
        return img.copy()
    a = img.astype(np.int64)
    s = 4 * a[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            s = s + a[dy:dy + h - 2, dx:dx + w - 2]
    out = img.copy()
    out[1:-1, 1:-1] = ((2 * s + 13) // 26).astype(np.uint8)
    return out


def _lut(img, tables):
    return np.stack([np.asarray(tables[c], dtype=np.uint8)[img[..., c]] for c in range(3)], axis=-1)


def autocontrast(img):
    tables = []
    for c in range(3):
        hist = np.bincount(img[..., c].reshape(-1), minlength=256)
        present = np.nonzero(hist)[0]
        lo, hi = int(present[0]), int(present[-1])
        if hi <= lo:
            tables.append(list(range(256)))
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        tables.append([min(255, max(0, int(ix * scale + offset))) for ix in range(256)])
    return _lut(img, tables)


def equalize(img):
    tables = []
    for c in range(3):
        hist = [int(v) for v in np.bincount(img[..., c].reshape(-1), minlength=256)]
        nz = [v for v in hist if v]
        step = (sum(nz) - nz[-1]) // 255 if len(nz) > 1 else 0
        if not step:
            tables.append(list(range(256)))
            continue
        n, lut = step // 2, []
        for i in range(256):
            lut.append(min(255, n // step))                   # Image.point clips its table to a byte
            n += hist[i]
        tables.append(lut)
    return _lut(img, tables)


def apply_op(img, op, fill=(0, 0, 0)):
    """one op on an HW3 uint8 image -> HW3 uint8"""
    code, factor, args = op
    if code == IDENTITY:
        return img.copy()
    if code == AFFINE:
        return affine(img, args, fill)
    if code == BRIGHTNESS:
        return R.apply_op(img, R.BRIGHTNESS, factor)
    if code == COLOR:
        return R.apply_op(img, R.SATURATION, factor)
    if code == CONTRAST:
        return R.apply_op(img, R.CONTRAST, factor)
    if code == SHARPNESS:
        return R.blend(smooth(img), img, factor)
    if code == POSTERIZE:
        return img & np.uint8(~((1 << (8 - int(args[0]))) - 1) & 255)
    if code == SOLARIZE:
        return np.where(img < int(args[0]), img, 255 - img).astype(np.uint8)
    if code == INVERT:
        return (255 - img).astype(np.uint8)
    if code == AUTOCONTRAST:
        return autocontrast(img)
    if code == EQUALIZE:
        return equalize(img)
    raise ValueError("unknown op %r" % (code,))


def chain(img, ops, fill=(0, 0, 0)):
    """the op chain of one MnasImgAug item on an HW3 uint8 image -> HW3 uint8"""
    img = np.asarray(img, dtype=np.uint8)
    for op in ops:
        img = apply_op(img, op, fill)
    return img.copy() if not ops else img


def policy_op(name, sign, index, bins, h, w):
    """RandAugment's magnitude table: the op ``name`` at magnitude ``index`` of ``bins`` linear steps, negated when ``sign`` is 1
    (signed ops only), on an h x w image -> (code, factor, args).  A zero magnitude is IDENTITY."""
    step = index / float(bins - 1) if bins > 1 else 0.0
    s = -1.0 if sign else 1.0
    ident = (IDENTITY, 0.0, ())
    if name == "Identity":
        return ident
    if name in ("ShearX", "ShearY"):
        m = s * 0.3 * step
        if m == 0.0:
            return ident
        return (AFFINE, 0.0, fixed_matrix((1, m, 0, 0, 1, 0) if name == "ShearX" else (1, 0, 0, m, 1, 0)))
    if name in ("TranslateX", "TranslateY"):
        t = int(s * (150.0 / 331.0 * (w if name == "TranslateX" else h)) * step)
        if t == 0:
            return ident
        return (AFFINE, 0.0, fixed_matrix((1, 0, t, 0, 1, 0) if name == "TranslateX" else (1, 0, 0, 0, 1, t)))
    if name == "Rotate":
        deg = s * 30.0 * step
        if deg == 0.0:
            return ident
        return (AFFINE, 0.0, fixed_matrix(rotate_matrix(deg, h, w)))
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        m = s * 0.9 * step
        if m == 0.0:
            return ident
        return ({"Brightness": BRIGHTNESS, "Color": COLOR, "Contrast": CONTRAST, "Sharpness": SHARPNESS}[name], 1.0 + m, ())
    if name == "Posterize":
        return (POSTERIZE, 0.0, (8 - int(round(4.0 * index / (bins - 1))) if bins > 1 else 8,))
    if name == "Solarize":
        return (SOLARIZE, 0.0, (int(math.ceil(255.0 - 255.0 * step)),))       # v < t for a real t is v < ceil(t)
    if name == "AutoContrast":
        return (AUTOCONTRAST, 0.0, ())
    if name == "Equalize":
        return (EQUALIZE, 0.0, ())
    if name == "Invert":                                                      # not one of RandAugment's 14: the AutoAugment policies' op
        return (INVERT, 0.0, ())
    raise ValueError(name)


def describe(n, hw, num_ops=2, magnitude=9, bins=31):
    """DeviceRandAugment.describe restated: per image and op position ``random.randrange(14)`` picks the op from NAMES, and a
    signed op then draws ``random.randrange(2)`` (1 negates) -> per image a list of (name, sign, (code, factor, args))"""
    out = []
    for _ in range(n):
        ops = []
        for _ in range(num_ops):
            name = NAMES[random.randrange(14)]
            sign = random.randrange(2) if name in SIGNED else 0
            ops.append((name, sign, policy_op(name, sign, magnitude, bins, hw[0], hw[1])))
        out.append(ops)
    return out


def pil_op(img, op, fill=(0, 0, 0), matrix=None):
    """the Pillow call an op is defined as (``matrix``: AFFINE's real-valued (a, b, c, d, e, f); imports PIL lazily)"""
    from PIL import Image, ImageEnhance, ImageOps
    code, factor, args = op
    im = Image.fromarray(np.ascontiguousarray(img), "RGB")
    if code == IDENTITY:
        out = im.copy()
    elif code == AFFINE:
        out = im.transform(im.size, Image.AFFINE, tuple(matrix), Image.NEAREST, fillcolor=tuple(int(v) for v in fill))
    elif code in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        enh = {BRIGHTNESS: ImageEnhance.Brightness, COLOR: ImageEnhance.Color, CONTRAST: ImageEnhance.Contrast,
               SHARPNESS: ImageEnhance.Sharpness}[code]
        out = enh(im).enhance(factor)
    elif code == POSTERIZE:
        out = ImageOps.posterize(im, int(args[0]))
    elif code == SOLARIZE:
        out = ImageOps.solarize(im, int(args[0]))
    elif code == INVERT:
        out = ImageOps.invert(im)
    elif code == AUTOCONTRAST:
        out = ImageOps.autocontrast(im)
    elif code == EQUALIZE:
        out = ImageOps.equalize(im)
    else:
        raise ValueError("unknown op %r" % (code,))
    return np.asarray(out).copy()


def pil_policy_op(img, name, sign, index, bins, fill=(0, 0, 0)):
    """the named policy op through Pillow alone (shears and translations by Image.transform, Rotate by Image.rotate)"""
    from PIL import Image
    h, w = img.shape[:2]
    step = index / float(bins - 1) if bins > 1 else 0.0
    s = -1.0 if sign else 1.0
    im = Image.fromarray(np.ascontiguousarray(img), "RGB")
    fc = tuple(int(v) for v in fill)
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
        if name.startswith("Shear"):
            m = s * 0.3 * step
            mat = (1, m, 0, 0, 1, 0) if name == "ShearX" else (1, 0, 0, m, 1, 0)
        else:
            t = int(s * (150.0 / 331.0 * (w if name == "TranslateX" else h)) * step)
            mat = (1, 0, t, 0, 1, 0) if name == "TranslateX" else (1, 0, 0, 0, 1, t)
        return np.asarray(im.transform(im.size, Image.AFFINE, mat, Image.NEAREST, fillcolor=fc)).copy()
    if name == "Rotate":
        return np.asarray(im.rotate(s * 30.0 * step, Image.NEAREST, fillcolor=fc)).copy()
    return pil_op(img, policy_op(name, sign, index, bins, h, w), fill)
