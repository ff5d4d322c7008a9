"""numpy restatement of the photometric image ops (csrc/mnas_imgc.hip, include/mnas.h MnasImgColor) and of the reference's
preprocessing type 3 built from them and tests/img_xform_ref.py.  Pillow's arithmetic, restated operation by operation (every
fp32 / fp64 operation rounded on its own, no FMA: numpy never contracts):

    grey      convert('L'):  L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16
    blend     ImageEnhance.*.enhance(f) = Image.blend(degenerate, img, f) (Blend.c), alpha = (float)f, per channel
              t = (float)a + alpha * (float)(b - a); 0 <= alpha <= 1: (uint8)t, else clipped to [0, 255] first
              degenerate a: 0 (Brightness), L of the pixel (Color), the rounded grey mean of the image (Contrast)
    hue       torchvision 0.2.x adjust_hue: RGB -> HSV (Convert.c rgb2hsv_row), H += shift mod 256, HSV -> RGB (hsv2rgb)
    gray      RandomGrayscale: (L, L, L)

tests/test_img_color_cpu.py holds every function here to the installed Pillow over its whole input domain.  ``pil_type3`` is
a literal Pillow restatement of the torchvision 0.2.x Compose for type 3 (the host route; imports PIL lazily).
"""
import random

import numpy as np

import img_xform_ref as X

BRIGHTNESS, CONTRAST, SATURATION, HUE, GRAY = 1, 2, 3, 4, 5        # MNAS_IMGC_*
NAMES = {BRIGHTNESS: "brightness", CONTRAST: "contrast", SATURATION: "saturation", HUE: "hue", GRAY: "gray"}


def grey(r, g, b):
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def blend(a, b, factor):
    """Image.blend(a, b, factor) per byte (a: the degenerate, b: the image), both uint8 arrays (a may broadcast)"""
    alpha = np.float32(factor)                               # _imaging.c: (float) of the Python float
    a = np.asarray(a).astype(np.int32)
    b = np.asarray(b).astype(np.int32)
    t = a.astype(np.float32) + alpha * (b - a).astype(np.float32)
    if 0.0 <= alpha <= 1.0:
        return t.astype(np.uint8)                             # (UINT8) of a value in [0, 255]: truncation
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64))).astype(np.uint8)


def contrast_mean(img):
    """ImageEnhance.Contrast's degenerate value: int(mean of convert('L') + 0.5), mean = exact sum / count in fp64"""
    L = grey(img[..., 0], img[..., 1], img[..., 2])
    s = int(L.astype(np.int64).sum())
    return int(float(s) / float(L.size) + 0.5)


def clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def rgb_to_hsv(r, g, b):
    """Convert.c rgb2hsv_row on uint8 arrays -> (H, S, V) uint8"""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    mx = np.maximum(r, np.maximum(g, b))
    mn = np.minimum(r, np.minimum(g, b))
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(np.float32)
    s = cr / np.where(mx == 0, 1, mx).astype(np.float32)                         # fp32 divisions
    rc = (mx - r).astype(np.float32) / cr
    gc = (mx - g).astype(np.float32) / cr
    bc = (mx - b).astype(np.float32) / cr
    h = np.where(r == mx, bc - gc,
                 np.where(g == mx, (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32),
                          (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)))
    x = h.astype(np.float64) / 6.0 + 1.0
    h = np.fmod(x, 1.0).astype(np.float32)
    H = clip8((h.astype(np.float64) * 255.0).astype(np.int64))                   # (int) truncates toward zero
    S = clip8((s.astype(np.float64) * 255.0).astype(np.int64))
    H = np.where(flat, 0, H).astype(np.uint8)
    S = np.where(flat, 0, S).astype(np.uint8)
    return H, S, mx.astype(np.uint8)


def _round(x):
    """C round(): half away from zero"""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def hsv_to_rgb(H, S, V):
    """Convert.c hsv2rgb on uint8 arrays -> (r, g, b) uint8"""
    H, S, V = (np.asarray(v).astype(np.int64) for v in (H, S, V))
    x = H.astype(np.float64) * 6.0 / 255.0
    i = np.floor(x).astype(np.int64)
    f = (x - i).astype(np.float32)
    fs = (S.astype(np.float64) / 255.0).astype(np.float32)
    v = V.astype(np.float64)
    p = clip8(_round(v * (1.0 - fs.astype(np.float64))).astype(np.int64))
    q = clip8(_round(v * (1.0 - (fs * f).astype(np.float64))).astype(np.int64))        # fs * f: an fp32 product
    t = clip8(_round(v * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64)))).astype(np.int64))
    V8 = V.astype(np.uint8)
    k = i % 6
    sel = [(V8, t, p), (q, V8, p), (p, V8, t), (p, q, V8), (t, p, V8), (V8, p, q)]
    out = []
    for c in range(3):
        o = np.select([k == j for j in range(6)], [sel[j][c] for j in range(6)])
        out.append(np.where(S == 0, V8, o).astype(np.uint8))
    return tuple(out)


def hue_shift(hue_factor):
    """torchvision 0.2.x np.uint8(hue_factor * 255) as numpy 1.x computed it: truncation toward zero, then mod 256"""
    return int(hue_factor * 255) % 256


def hue(img, shift):
    H, S, V = rgb_to_hsv(img[..., 0], img[..., 1], img[..., 2])
    H = ((H.astype(np.int64) + int(shift)) & 255).astype(np.uint8)
    return np.stack(hsv_to_rgb(H, S, V), axis=-1)


def apply_op(img, op, factor=0.0, shift=0):
    """one op on an (..., H, W, 3) uint8 image (one image: contrast takes the whole array's mean)"""
    if op == BRIGHTNESS:
        return blend(np.uint8(0), img, factor)
    if op == CONTRAST:
        return blend(np.uint8(contrast_mean(img)), img, factor)
    if op == SATURATION:
        L = grey(img[..., 0], img[..., 1], img[..., 2])
        return blend(L[..., None], img, factor)
    if op == HUE:
        return hue(img, shift)
    if op == GRAY:
        L = grey(img[..., 0], img[..., 1], img[..., 2])
        return np.repeat(L[..., None], 3, axis=-1)
    raise ValueError("unknown op %r" % op)


def color(img, ops, factors=(), shift=0):
    """the op chain of one MnasImgColor item on an HW3 uint8 image -> HW3 uint8"""
    img = np.asarray(img, dtype=np.uint8)
    factors = list(factors) + [0.0] * (len(ops) - len(factors))
    for op, f in zip(ops, factors):
        img = apply_op(img, op, f, shift)
    return img


class CubeTables:
    """RGB -> HSV over all 2^24 RGB triples and HSV -> RGB over all 2^24 HSV triples, as uint8 (2^24, 3) tables indexed by
    (a << 16) | (b << 8) | c: a whole-cube hue is two gathers (the GPU tests check 2^24-pixel images this way)."""

    def __init__(self, chunk=1 << 21):
        n = 1 << 24
        self.hsv = np.empty((n, 3), np.uint8)
        self.rgb = np.empty((n, 3), np.uint8)
        for o in range(0, n, chunk):
            idx = np.arange(o, o + chunk, dtype=np.int64)
            a, b, c = idx >> 16, (idx >> 8) & 255, idx & 255
            self.hsv[o:o + chunk] = np.stack(rgb_to_hsv(a, b, c), axis=-1)
            self.rgb[o:o + chunk] = np.stack(hsv_to_rgb(a, b, c), axis=-1)

    @staticmethod
    def index(img):
        img = img.astype(np.int64)
        return (img[..., 0] << 16) | (img[..., 1] << 8) | img[..., 2]

    def hue(self, img, shift):
        hsv = self.hsv[self.index(img)].astype(np.int64)
        hsv[..., 0] = (hsv[..., 0] + int(shift)) & 255
        return self.rgb[(hsv[..., 0] << 16) | (hsv[..., 1] << 8) | hsv[..., 2]]


def cube_image():
    """all 2^24 RGB triples as one 4096 x 4096 HW3 uint8 image, pixel k = (k >> 16, (k >> 8) & 255, k & 255)"""
    k = np.arange(1 << 24, dtype=np.int64)
    return np.stack([k >> 16, (k >> 8) & 255, k & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


# ---- preprocessing type 3 (datasets.py preprocess_img) ----
def jitter_params(brightness=0.1, contrast=0.1, saturation=0.1, hue_=0.1):
    """torchvision 0.2.x ColorJitter.get_params: [(op, factor)] in the shuffled order (module-level random)"""
    ops = []
    if brightness > 0:
        ops.append((BRIGHTNESS, random.uniform(max(0, 1 - brightness), 1 + brightness)))
    if contrast > 0:
        ops.append((CONTRAST, random.uniform(max(0, 1 - contrast), 1 + contrast)))
    if saturation > 0:
        ops.append((SATURATION, random.uniform(max(0, 1 - saturation), 1 + saturation)))
    if hue_ > 0:
        ops.append((HUE, random.uniform(-hue_, hue_)))
    random.shuffle(ops)
    return ops


def jitter(img, ops):
    """ColorJitter with drawn [(op, factor)] (hue factors in [-0.5, 0.5]) on an HW3 uint8 image"""
    for op, f in ops:
        img = apply_op(img, op, f, hue_shift(f) if op == HUE else 0)
    return img


def type3(img, final_size, draw):
    """one image of preprocessing type 3 from its draws (DevicePipeline.describe's per-image record) -> (3, fh, fw) uint8"""
    fh, fw = final_size
    rgb = X.to_rgb(img)
    h, w = rgb.shape[:2]
    x = X.xform(rgb, (0, 0, h, w), (fh, fw), (0, 0), (fh, fw)).transpose(1, 2, 0)         # Resize(final_size)
    box = (0, 0, fh, fw)
    if draw.applied:
        x = jitter(x, draw.jitter)
        box = draw.box
    x = X.xform(x, box, (fh, fw), (0, 0), (fh, fw), draw.flags)                           # identity resample when not applied
    if draw.gray:
        x = apply_op(x.transpose(1, 2, 0), GRAY).transpose(2, 0, 1)
    return np.ascontiguousarray(x)


def pil_type3(img, final_size, prob=0.2):
    """The torchvision 0.2.x Compose of preprocessing type 3 on Pillow, drawing from the module-level random (needs PIL):
        Resize(final_size), RandomApply([ColorJitter(.1, .1, .1, .1), RandomResizedCropRect(final_size, (0.7, 1.0),
        (0.7, 1.2))], p=prob), RandomHorizontalFlip(prob), RandomVerticalFlip(prob), RandomGrayscale(prob)
    -> (3, fh, fw) uint8 (the ToTensor / Normalize tail is left out)."""
    from PIL import Image, ImageEnhance
    from mnasnet_pytorch_amd.transforms import get_params
    bilinear = getattr(Image, "Resampling", Image).BILINEAR
    fh, fw = final_size
    im = Image.fromarray(X.to_rgb(img), "RGB").resize((fw, fh), bilinear)

    def adjust_hue(im, f):
        h, s, v = im.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        np_h += np.uint8(hue_shift(f))                        # 0.2.x: np.uint8(f * 255), numpy 1.x wrap-around
        return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")

    if not prob < random.random():                            # RandomApply
        for op, f in jitter_params():
            if op == BRIGHTNESS:
                im = ImageEnhance.Brightness(im).enhance(f)
            elif op == CONTRAST:
                im = ImageEnhance.Contrast(im).enhance(f)
            elif op == SATURATION:
                im = ImageEnhance.Color(im).enhance(f)
            else:
                im = adjust_hue(im, f)
        i, j, h, w = get_params(fh, fw, (0.7, 1.0), (0.7, 1.2))
        im = im.crop((j, i, j + w, i + h)).resize((fw, fh), bilinear)
    flip = getattr(Image, "Transpose", Image)
    if random.random() < prob:
        im = im.transpose(flip.FLIP_LEFT_RIGHT)
    if random.random() < prob:
        im = im.transpose(flip.FLIP_TOP_BOTTOM)
    if random.random() < prob:
        L = np.array(im.convert("L"), dtype=np.uint8)
        im = Image.fromarray(np.dstack([L, L, L]), "RGB")
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def pil_op(img, op, factor=0.0, shift=0):
    """one op through Pillow on an HW3 uint8 image (the oracle of apply_op; needs PIL)"""
    from PIL import Image, ImageEnhance
    im = Image.fromarray(np.ascontiguousarray(img), "RGB")
    if op == BRIGHTNESS:
        im = ImageEnhance.Brightness(im).enhance(factor)
    elif op == CONTRAST:
        im = ImageEnhance.Contrast(im).enhance(factor)
    elif op == SATURATION:
        im = ImageEnhance.Color(im).enhance(factor)
    elif op == HUE:
        h, s, v = im.convert("HSV").split()
        np_h = (np.array(h, dtype=np.int64) + shift) & 255
        im = Image.merge("HSV", (Image.fromarray(np_h.astype(np.uint8), "L"), s, v)).convert("RGB")
    elif op == GRAY:
        L = np.array(im.convert("L"), dtype=np.uint8)
        return np.dstack([L, L, L])
    return np.asarray(im)

