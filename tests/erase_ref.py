"""CPU restatement of Random Erasing on uint8 batches (mnasnet_pytorch_amd/erasing.py, include/mnas.h "device random numbers" /
"Random Erasing"), written from the header's rules: Philox4x32-10 in numpy uint64 arithmetic, the quantile table from
statistics.NormalDist, the erase pixel by pixel over whole boxes, the draws from the documented order.  tests/test_erase_cpu.py
holds the known answers, the table and the draw order to it; the GPU tests compare the kernel with it."""
import math
import random
from statistics import NormalDist

import numpy as np

NONE, CONST, NOISE = 0, 1, 2
TABLE = 4096
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# counter, key -> output (include/mnas.h)
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words held in uint64 -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                 # < 2^64: exact
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def table(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(3, 4096) uint8: T_c[i] = clamp(floor(255 (mean_c + std_c Phi^-1((i + 0.5) / 4096)) + 0.5), 0, 255)"""
    q = [NormalDist().inv_cdf((i + 0.5) / TABLE) for i in range(TABLE)]
    return np.array([[min(max(math.floor(255.0 * (m + s * v) + 0.5), 0), 255) for v in q] for m, s in zip(mean, std)], dtype=np.uint8)


def noise_bytes(tab, seed, position, n, c, ys, xs):
    """the NOISE bytes of plane c of image n at rows ys x columns xs (image coordinates) -> (len(ys), len(xs)) uint8"""
    y, x = np.meshgrid(np.asarray(ys, dtype=np.uint64), np.asarray(xs, dtype=np.uint64), indexing="ij")
    r = philox(x >> np.uint64(3), y, 3 * n + c, position, seed & 0xFFFFFFFF, seed >> 32)
    word = np.choose(((x & np.uint64(7)) >> np.uint64(1)).astype(np.int64), r)
    half = np.where((x & np.uint64(1)) == 1, word >> np.uint64(16), word & np.uint64(0xFFFF))
    return np.asarray(tab).reshape(3, TABLE)[c][(half & np.uint64(TABLE - 1)).astype(np.int64)]


def erase_position(x, items, tab, seed, position):
    """one launch: x (n, 3, H, W) uint8, changed in place; items: (mode, (y0, x0, y1, x1), fill) per image"""
    for n, (mode, (y0, x0, y1, x1), fill) in enumerate(items):
        if mode == NONE or y1 <= y0 or x1 <= x0:
            continue
        for c in range(3):
            if mode == CONST:
                x[n, c, y0:y1, x0:x1] = fill[c]
            else:
                x[n, c, y0:y1, x0:x1] = noise_bytes(tab, seed, position, n, c, range(y0, y1), range(x0, x1))
    return x


def position_items(draws, position):
    """draws[k]: image k's boxes -> the items of one box position (an image with fewer boxes: NONE)"""
    return [tuple(b[position]) if position < len(b) else (NONE, (0, 0, 0, 0), (0, 0, 0)) for b in draws]


def erase_batch(x, draws, tab, seed):
    """every position in order on a copy of x -> the erased batch"""
    out = x.copy()
    for p in range(max((len(b) for b in draws), default=0)):
        erase_position(out, position_items(draws, p), tab, seed, p)
    return out


def describe(n, h, w, prob=0.25, min_area=0.02, max_area=1.0 / 3.0, min_aspect=0.3, max_aspect=None, mode="pixel", value=(0, 0, 0),
             min_count=1, max_count=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """DeviceRandomErasing.describe from its documented draw order -> ([[(mode, box, fill), ...] per image], seed)"""
    max_aspect = 1.0 / min_aspect if max_aspect is None else max_aspect
    max_count = min_count if max_count is None else max_count
    tab = table(mean, std)
    draws = []
    for _ in range(n):
        boxes = []
        if random.random() < prob:
            count = min_count if min_count == max_count else random.randint(min_count, max_count)
            for _ in range(count):
                for _ in range(10):
                    area = random.uniform(min_area, max_area) * h * w / count
                    aspect = math.exp(random.uniform(math.log(min_aspect), math.log(max_aspect)))
                    bh = int(round(math.sqrt(area * aspect)))
                    bw = int(round(math.sqrt(area / aspect)))
                    if bw < w and bh < h:
                        top = random.randint(0, h - bh)
                        left = random.randint(0, w - bw)
                        fill = tuple(value)
                        if mode == "rand":
                            fill = tuple(int(tab[c][random.getrandbits(12)]) for c in range(3))
                        if bh > 0 and bw > 0:
                            boxes.append((NOISE if mode == "pixel" else CONST, (top, left, top + bh, left + bw), fill))
                        break
        draws.append(boxes)
    return draws, random.getrandbits(64)
