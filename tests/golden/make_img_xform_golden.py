"""Generates tests/golden/img_xform.npz: small decoded images and what Pillow's crop + BILINEAR resize (+ window, flips) makes
of them -- the fixture the image batch transform (csrc/mnas_imgx.hip) is held to on the GPU, where Pillow may not exist.  Run:
    python tests/golden/make_img_xform_golden.py
Sources are <= 160 x 120, a closed-form integer pattern plus stored noise, C = 1 / 3 / 4.  The cases cover upscaling, 8x, 20x
and 32x downscaling, the identity size, 1-pixel boxes and outputs, windows and both flips; ``e2e`` is one 8-image 64 x 64 batch
of RandomResizedCrop + horizontal-flip descriptors (the end-to-end model test).

Arrays: src (uint8, sources back to back, 16-byte padded), src_meta (int64 [S][4]: offset, h, w, c), cases (int64 [K][12]:
src, box_top, box_left, box_h, box_w, rh, rw, win_top, win_left, flags, Ho, Wo), out (uint8, outputs back to back, NCHW per
case), out_off (int64 [K]), e2e_cases (int64 [8][12]), e2e_out (uint8 [8][3][64][64])."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import img_xform_ref as R  # noqa: E402

SOURCES = [(120, 160, 3), (160, 120, 1), (97, 131, 4), (64, 48, 3)]

# src, (box_top, box_left, box_h, box_w), (rh, rw), (win_top, win_left), flags, (Ho, Wo)
CASES = [
    (3, (0, 0, 64, 48), (64, 48), (0, 0), 0, (64, 48)),                 # identity size
    (3, (10, 5, 20, 15), (50, 37), (0, 0), 0, (50, 37)),                # upscale
    (0, (30, 40, 16, 16), (64, 64), (10, 12), 0, (32, 40)),             # upscale, window
    (0, (0, 0, 120, 160), (15, 20), (0, 0), 3, (15, 20)),               # 8x downscale, both flips
    (1, (0, 0, 160, 120), (8, 6), (0, 0), 1, (8, 6)),                   # 20x, grey
    (2, (0, 0, 97, 131), (5, 7), (0, 0), 2, (5, 7)),                    # ~20x, alpha dropped
    (1, (0, 0, 160, 120), (5, 4), (0, 0), 0, (5, 4)),                   # 32x / 30x: the largest supported downscale
    (0, (50, 60, 1, 1), (7, 5), (0, 0), 0, (7, 5)),                     # 1-pixel box
    (2, (3, 4, 1, 9), (4, 9), (1, 2), 1, (3, 6)),                       # 1-pixel-high box, window, hflip
    (3, (10, 5, 20, 15), (1, 1), (0, 0), 0, (1, 1)),                    # 1-pixel output
    (2, (10, 10, 80, 20), (20, 60), (0, 0), 2, (20, 60)),               # down one axis, up the other
    (1, (20, 10, 100, 90), (45, 50), (5, 7), 3, (33, 40)),              # grey, window, both flips
    (2, (0, 0, 97, 131), (120, 150), (50, 60), 1, (24, 32)),            # alpha, upscale, window, hflip
    (0, (7, 9, 101, 143), (61, 97), (0, 0), 1, (61, 97)),               # odd sizes
    (3, (0, 0, 64, 48), (64, 48), (3, 5), 2, (40, 30)),                 # identity size, window, vflip
    (0, (1, 2, 117, 157), (13, 157), (0, 0), 0, (13, 157)),             # width unchanged, height 9x
]


def source(h, w, c, noise):
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    return ((x * 7 + y * 13 + ch * 85 + (x * y) // 5 + noise) & 255).astype(np.uint8)


def e2e_cases():
    from mnasnet_pytorch_amd.transforms import get_params
    random.seed(20261016)
    out = []
    for k in range(8):
        s = k % len(SOURCES)
        h, w, _ = SOURCES[s]
        box = get_params(h, w)
        out.append((s, box, (64, 64), (0, 0), 1 if random.random() < 0.5 else 0, (64, 64)))
    return out


def row(case):
    s, box, rs, win, flags, hw = case
    return [s, *box, *rs, *win, flags, *hw]


def run(case, srcs):
    s, box, rs, win, flags, hw = case
    a = R.pil_xform(srcs[s], box, rs, win, hw, flags)
    b = R.xform(srcs[s], box, rs, win, hw, flags)
    assert np.array_equal(a, b), case            # the restatement agrees with Pillow on every stored case
    return a


def main():
    rng = np.random.default_rng(1234)
    srcs = [source(h, w, c, rng.integers(0, 32, (h, w, c))) for h, w, c in SOURCES]
    meta, off = [], 0
    for a in srcs:
        meta.append((off, *a.shape))
        off += a.nbytes
    buf = np.zeros((off + 15) & ~15, dtype=np.uint8)
    for a, m in zip(srcs, meta):
        buf[m[0]:m[0] + a.nbytes] = a.reshape(-1)
    outs = [run(c, srcs) for c in CASES]
    out_off = np.cumsum([0] + [o.size for o in outs[:-1]]).astype(np.int64)
    e2e = e2e_cases()
    e2e_out = np.stack([run(c, srcs) for c in e2e])
    path = os.path.join(HERE, "img_xform.npz")
    np.savez_compressed(path, src=buf, src_meta=np.array(meta, dtype=np.int64),
                        cases=np.array([row(c) for c in CASES], dtype=np.int64),
                        out=np.concatenate([o.reshape(-1) for o in outs]), out_off=out_off,
                        e2e_cases=np.array([row(c) for c in e2e], dtype=np.int64), e2e_out=e2e_out)
    print("wrote %s (%d bytes, %d cases + %d-image batch)" % (path, os.path.getsize(path), len(CASES), len(e2e)))


if __name__ == "__main__":
    main()
