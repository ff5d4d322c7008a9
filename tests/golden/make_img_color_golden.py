"""Generates tests/golden/img_color.npz: what Pillow makes of small uint8 images under the photometric ops -- the fixture the
photometric image kernels (csrc/mnas_imgc.hip) are held to on the GPU, where Pillow may not exist.  Run:
    python tests/golden/make_img_color_golden.py
``op_*``: one 40 x 56 RGB source (a closed-form pattern plus stored noise, with flat grey patches for the S = 0 branches) through
every op alone at factors on both sides of 1 and hue shifts that wrap, and through chains of all four jitter ops.  ``t3_*``: a
seeded batch of preprocessing type 3 at prob 0.5 (mixed source sizes and channel counts, final size 36 x 52), built by the
literal Pillow Compose (img_color_ref.pil_type3); the GPU test replays the same seed through DevicePipeline.

Arrays: op_src (uint8 [40][56][3]), op_cases (float64 [K][12]: nops, op[5], factor[5], hue_shift), op_out (uint8 [K][40][56][3]),
t3_src (uint8, sources back to back, 16-byte padded), t3_meta (int64 [S][4]: offset, h, w, c), t3_seed, t3_prob, t3_size,
t3_out (uint8 [S][3][36][52])."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import img_color_ref as R  # noqa: E402

B, C, S, H, G = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE, R.GRAY

# (ops, factors, hue_shift)
OP_CASES = [
    ([B], [0.0], 0), ([B], [0.8], 0), ([B], [1.0], 0), ([B], [1.1], 0), ([B], [3.7], 0),
    ([C], [0.0], 0), ([C], [0.9], 0), ([C], [1.1], 0), ([C], [2.5], 0),
    ([S], [0.0], 0), ([S], [0.9], 0), ([S], [1.1], 0), ([S], [4.0], 0),
    ([H], [0.0], 1), ([H], [0.0], 25), ([H], [0.0], 128), ([H], [0.0], 231), ([H], [0.0], 255),
    ([G], [0.0], 0),
    ([H, S, B, C], [0.0, 1.07, 0.93, 1.02], 243),                   # contrast last: its mean sees the three ops before it
    ([C, B, H, S], [0.95, 1.04, 0.0, 0.91], 12),
    ([S, C, H, B], [1.09, 0.97, 0.0, 1.1], 251),
    ([B, S, C, H, G], [1.05, 0.92, 1.08, 0.0, 0.0], 7),
]
T3_SOURCES = [(50, 70, 3), (36, 52, 3), (61, 45, 1), (30, 80, 4), (44, 44, 3), (72, 50, 3), (40, 60, 1), (36, 52, 4)]
T3_SEED, T3_PROB, T3_SIZE = 20261016, 0.5, (36, 52)


def source(h, w, c, noise):
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return ((x * 11 + y * 5 + ch * 70 + (x * y) // 7 + noise) & 255).astype(np.uint8)


def pil_chain(img, ops, factors, shift):
    for op, f in zip(ops, factors):
        img = R.pil_op(img, op, f, shift)
    return img


def main():
    rng = np.random.default_rng(77)
    src = source(40, 56, 3, rng.integers(0, 48, (40, 56, 3)))
    src[4:10, 4:12] = 128                                             # flat patches: H = S = 0
    src[20:24, 30:40] = 255
    src[30:34, 8:14] = 0
    rows, outs = [], []
    for ops, fac, shift in OP_CASES:
        want = pil_chain(src, ops, fac, shift)
        assert np.array_equal(R.color(src, ops, fac, shift), want), (ops, fac, shift)
        rows.append([len(ops)] + ops + [0] * (5 - len(ops)) + fac + [0.0] * (5 - len(fac)) + [shift])
        outs.append(want)
    t3 = [source(h, w, c, rng.integers(0, 64, (h, w, c))) for h, w, c in T3_SOURCES]
    meta, off = [], 0
    for a in t3:
        meta.append((off, *a.shape))
        off += a.nbytes
    buf = np.zeros((off + 15) & ~15, dtype=np.uint8)
    for a, m in zip(t3, meta):
        buf[m[0]:m[0] + a.nbytes] = a.reshape(-1)
    random.seed(T3_SEED)
    t3_out = np.stack([R.pil_type3(a, T3_SIZE, T3_PROB) for a in t3])
    path = os.path.join(HERE, "img_color.npz")
    np.savez_compressed(path, op_src=src, op_cases=np.array(rows, dtype=np.float64), op_out=np.stack(outs), t3_src=buf,
                        t3_meta=np.array(meta, dtype=np.int64), t3_seed=T3_SEED, t3_prob=T3_PROB,
                        t3_size=np.array(T3_SIZE, dtype=np.int64), t3_out=t3_out)
    print("wrote %s (%d bytes, %d op cases + %d-image type-3 batch)" % (path, os.path.getsize(path), len(rows), len(t3)))


if __name__ == "__main__":
    main()
