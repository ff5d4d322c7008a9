"""Generates tests/golden/randaug.npz: what Pillow makes of small uint8 images under the augmentation-policy ops -- the fixture
the kernels of csrc/mnas_imga.hip are held to on the GPU, where Pillow may not exist.  Run:
    python tests/golden/make_randaug_golden.py
``src``: two 24 x 40 RGB sources, a closed-form pattern plus stored noise and a low-contrast copy of it (so that AutoContrast and
Equalize have work to do).  ``op_*``: every policy op alone at two magnitudes and both signs (plus Invert), through Pillow's own
calls (Image.transform, Image.rotate, ImageEnhance, ImageOps).  ``chain_*``: two-op chains, Equalize then AutoContrast among them.
``ra_*``: one seeded DeviceRandAugment(2, 9).describe over eight images with its descriptors and Pillow's bytes.

Arrays: src (uint8 [2][24][40][3]), fill (uint8 [3]), op_cases (float64 [K][9]: source, op code, factor, six integer arguments),
op_out (uint8 [K][24][40][3]), chain_cases (float64 [C][2][9], same columns per op), chain_out (uint8 [C][24][40][3]), ra_seed,
ra_src (int64 [8]: the source of each image), ra_cases (float64 [8][2][9]), ra_out (uint8 [8][24][40][3])."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import randaug_ref as A  # noqa: E402

H, W, BINS = 24, 40, 31
FILL = (7, 130, 255)
MAGNITUDES = [(0, 9), (1, 24)]                                       # (sign, step of 31)
# (source, [(name, sign, step)])
CHAINS = [
    (1, [("Equalize", 0, 9), ("AutoContrast", 0, 9)]),                # the second statistics pass reads the first's output
    (0, [("Rotate", 1, 20), ("Contrast", 0, 15)]),
    (0, [("Sharpness", 0, 30), ("ShearX", 1, 30)]),
    (1, [("AutoContrast", 0, 0), ("Solarize", 0, 12)]),
    (0, [("TranslateY", 0, 18), ("Posterize", 0, 30)]),
    (1, [("Color", 1, 27), ("Invert", 0, 0)]),
]
RA_SEED, RA_N = 20261020, 8


def sources():
    rng = np.random.default_rng(41)
    y, x, ch = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    a = ((x * 9 + y * 7 + ch * 80 + (x * y) // 5 + rng.integers(0, 40, (H, W, 3))) & 255).astype(np.uint8)
    return np.stack([a, (a // 3 + 60).astype(np.uint8)])


def row(src, op):
    code, factor, args = op
    return [src, code, factor] + [int(v) for v in args] + [0] * (6 - len(args))


def build():
    """every array of the fixture, from Pillow; the restatement must agree case by case"""
    src = sources()
    op_cases, op_out = [], []
    for name in A.NAMES + ["Invert"]:
        for k, (sign, step) in enumerate(MAGNITUDES):
            s = (k + (name in ("AutoContrast", "Equalize"))) % 2       # the low-contrast source for both statistics tables
            op = A.policy_op(name, sign, step, BINS, H, W)
            want = A.pil_policy_op(src[s], name, sign, step, BINS, FILL)
            assert np.array_equal(A.apply_op(src[s], op, FILL), want), (name, sign, step)
            op_cases.append(row(s, op))
            op_out.append(want)
    chain_cases, chain_out = [], []
    for s, names in CHAINS:
        img, ops = src[s], []
        for name, sign, step in names:
            img = A.pil_policy_op(img, name, sign, step, BINS, FILL)
            ops.append(A.policy_op(name, sign, step, BINS, H, W))
        assert np.array_equal(A.chain(src[s], ops, FILL), img), names
        chain_cases.append([row(s, op) for op in ops])
        chain_out.append(img)
    random.seed(RA_SEED)
    draws = A.describe(RA_N, (H, W), 2, 9, BINS)
    ra_src = [k % 2 for k in range(RA_N)]
    ra_cases, ra_out = [], []
    for s, ops in zip(ra_src, draws):
        img = src[s]
        for name, sign, _ in ops:
            img = A.pil_policy_op(img, name, sign, 9, BINS, FILL)
        assert np.array_equal(A.chain(src[s], [op for _, _, op in ops], FILL), img), ops
        ra_cases.append([row(s, op) for _, _, op in ops])
        ra_out.append(img)
    return dict(src=src, fill=np.array(FILL, dtype=np.uint8), op_cases=np.array(op_cases, dtype=np.float64),
                op_out=np.stack(op_out), chain_cases=np.array(chain_cases, dtype=np.float64), chain_out=np.stack(chain_out),
                ra_seed=np.int64(RA_SEED), ra_src=np.array(ra_src, dtype=np.int64), ra_cases=np.array(ra_cases, dtype=np.float64),
                ra_out=np.stack(ra_out))


def main(path=None):
    path = path or os.path.join(HERE, "randaug.npz")
    arrays = build()
    np.savez_compressed(path, **arrays)
    print("wrote %s (%d bytes, %d op cases, %d chains, %d-image RandAugment batch)"
          % (path, os.path.getsize(path), len(arrays["op_cases"]), len(arrays["chain_cases"]), len(arrays["ra_cases"])))


if __name__ == "__main__":
    main()
