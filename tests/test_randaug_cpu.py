"""CPU (no GPU needed): the augmentation-policy ops' host half.  The numpy restatement (tests/randaug_ref.py) equals Pillow for
every op -- the nearest-neighbour affine warp over 300+ random shears, rotations and translations, the SMOOTH filter behind
Sharpness, the enhancers, posterize / solarize / invert, and the AutoContrast and Equalize tables on constant, two-valued,
fewer-than-255-pixel and ordinary channels -- on images of sizes (1, 5), (2, 7), (3, 3), (37, 29) and (64, 96);
DeviceRandAugment.describe makes the restatement's draws and reproduces the golden descriptors; the golden's chains are Pillow's
bytes and the file regenerates from its script; mnas_img_aug_check refuses every kind of bad item (host function only: nothing
here launches a kernel)."""
import ctypes
import math
import os
import random

import numpy as np
import pytest

import cases as C
import randaug_ref as A

G = os.path.join(C.GOLDEN_DIR, "randaug.npz")
SIZES = [(1, 5), (2, 7), (3, 3), (37, 29), (64, 96)]
FILL = (9, 200, 77)


def _images(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]


def _ops(rows):
    """golden rows (source, code, factor, six arguments) -> [(source, (code, factor, args))]"""
    return [(int(r[0]), (int(r[1]), float(r[2]), tuple(int(v) for v in r[3:9]))) for r in rows]


def test_affine_against_pillow():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(1)
    n = 0
    for img in _images(2):
        h, w = img.shape[:2]
        mats = []
        for _ in range(25):
            m = float(rng.uniform(-1.2, 1.2))
            mats.append((1, m, 0, 0, 1, 0))
            mats.append((1, 0, 0, m, 1, 0))
            mats.append(A.rotate_matrix(float(rng.uniform(-179.0, 179.0)), h, w))
        for _ in range(8):
            mats.append((1, 0, int(rng.integers(-w - 1, w + 2)), 0, 1, 0))
            mats.append((1, 0, 0, 0, 1, int(rng.integers(-h - 1, h + 2))))
            mats.append((1, 0, int(rng.integers(-w, w + 1)), 0, 1, int(rng.integers(-h, h + 1))))
        for m in mats:
            op = (A.AFFINE, 0.0, A.fixed_matrix(m))
            assert np.array_equal(A.apply_op(img, op, FILL), A.pil_op(img, op, FILL, matrix=m)), (h, w, m)
            n += 1
    assert n >= 300
    with pytest.raises(ValueError):
        A.fixed_matrix((1.5, 0, 0, 0, 1, 0))                        # b == d == 0: Pillow's other route, defined for translations only
    with pytest.raises(ValueError):
        A.fixed_matrix((1, 0, 0.5, 0, 1, 0))


def test_policy_ops_against_pillow():
    """all 14 named ops, both signs, through Pillow's own entry points (Image.rotate for Rotate) at the ends and inside the table"""
    pytest.importorskip("PIL")
    for img in _images(3):
        h, w = img.shape[:2]
        for name in A.NAMES:
            for sign in (0, 1):
                for step in (0, 9, 17, 30):
                    op = A.policy_op(name, sign, step, 31, h, w)
                    assert np.array_equal(A.apply_op(img, op, FILL), A.pil_policy_op(img, name, sign, step, 31, FILL)), (h, w, name, sign, step)
    assert A.policy_op("ShearX", 0, 0, 31, 8, 8)[0] == A.IDENTITY and A.policy_op("TranslateX", 1, 1, 31, 8, 8)[0] == A.IDENTITY
    assert [A.policy_op("Posterize", 0, i, 31, 8, 8)[2][0] for i in (0, 3, 4, 11, 12, 19, 26, 27, 30)] == [8, 8, 7, 7, 6, 5, 5, 4, 4]
    assert [A.policy_op("Solarize", 0, i, 31, 8, 8)[2][0] for i in (0, 9, 30)] == [255, 179, 0]


def test_pointwise_ops_and_the_filter_against_pillow():
    pytest.importorskip("PIL")
    from PIL import Image, ImageFilter
    for img in _images(4):
        assert np.array_equal(A.smooth(img), np.asarray(Image.fromarray(img, "RGB").filter(ImageFilter.SMOOTH))), img.shape
        ops = [(A.SHARPNESS, f, ()) for f in (0.1, 1.0, 1.9, 0.0, 0.55)]
        ops += [(code, f, ()) for code in (A.BRIGHTNESS, A.COLOR, A.CONTRAST) for f in (0.1, 0.73, 1.0, 1.27, 1.9)]
        ops += [(A.POSTERIZE, 0.0, (bits,)) for bits in range(1, 9)]
        ops += [(A.SOLARIZE, 0.0, (t,)) for t in (0, 1, 128, 255, 256)]
        ops += [(A.INVERT, 0.0, ()), (A.IDENTITY, 0.0, ())]
        for op in ops:
            assert np.array_equal(A.apply_op(img, op), A.pil_op(img, op)), (img.shape, op)


def test_autocontrast_and_equalize_tables_against_pillow():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(5)
    imgs = _images(6)                                               # three of them have fewer than 255 pixels: equalize's step is 0
    assert sum(a.shape[0] * a.shape[1] < 255 for a in imgs) == 3
    for h, w in [(37, 29), (64, 96), (3, 3)]:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        a[..., 1] = 93                                              # a constant channel
        a[..., 2] = np.where(rng.random((h, w)) < 0.3, 40, 200)     # a two-valued channel
        imgs.append(a)
        imgs.append((rng.integers(0, 256, (h, w, 3)) // 4 + 100).astype(np.uint8))       # low contrast: lo > 0, hi < 255
        b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b[..., 0] = np.where(rng.random((h, w)) < 0.5, 0, 255)
        b[..., 1] = np.where(rng.random((h, w)) < 0.999, 17, 18)    # two values, one of them rare
        imgs.append(b)
    imgs.append(np.full((40, 40, 3), 255, dtype=np.uint8))
    imgs.append(np.zeros((40, 40, 3), dtype=np.uint8))
    clipped = 0
    for a in imgs:
        for code in (A.AUTOCONTRAST, A.EQUALIZE):
            assert np.array_equal(A.apply_op(a, (code, 0.0, ())), A.pil_op(a, (code, 0.0, ()))), (a.shape, code)
        for c in range(3):                                          # equalize tables whose last entry Image.point clips from 256
            hist = np.bincount(a[..., c].reshape(-1), minlength=256)
            nz = hist[hist > 0]
            step = (int(nz.sum()) - int(nz[-1])) // 255 if len(nz) > 1 else 0
            clipped += bool(step) and (step // 2 + int(nz.sum()) - int(nz[-1])) // step > 255
    assert clipped > 0


def test_restatement_equals_the_golden():
    g = np.load(G)
    src, fill = g["src"], tuple(int(v) for v in g["fill"])
    for (s, op), want in zip(_ops(g["op_cases"]), g["op_out"]):
        assert np.array_equal(A.apply_op(src[s], op, fill), want), op
    assert {op[0] for _, op in _ops(g["op_cases"])} == set(range(11))                      # every op code of the kernel
    for rows, want in list(zip(g["chain_cases"], g["chain_out"])) + list(zip(g["ra_cases"], g["ra_out"])):
        ops = _ops(rows)
        assert np.array_equal(A.chain(src[ops[0][0]], [op for _, op in ops], fill), want), ops
    assert os.path.getsize(G) < os.path.getsize(os.path.join(C.GOLDEN_DIR, "img_color.npz"))


def test_describe_reproduces_the_golden_descriptors():
    from mnasnet_pytorch_amd import DeviceRandAugment
    g = np.load(G)
    h, w = g["src"].shape[1:3]
    seed, n = int(g["ra_seed"]), len(g["ra_cases"])
    random.seed(seed)
    rows = DeviceRandAugment(2, 9).describe(n, (h, w))
    after = random.random()
    random.seed(seed)
    ref = A.describe(n, (h, w), 2, 9, 31)
    assert random.random() == after                                 # the same number of draws
    for mine, theirs, gold in zip(rows, ref, g["ra_cases"]):
        assert len(mine) == 2
        for o, (name, sign, op), (_, gop) in zip(mine, theirs, _ops(gold)):
            got = (o.op, o.factor, tuple(o.args) + (0,) * (6 - len(o.args)))
            assert (o.name, o.sign) == (name, sign) and got == (op[0], op[1], tuple(op[2]) + (0,) * (6 - len(op[2]))) == gop
    # the draw order: randrange(14), then randrange(2) for the signed ops only
    random.seed(77)
    picks = []
    for _ in range(40):
        k = random.randrange(14)
        picks.append((A.NAMES[k], random.randrange(2) if 1 <= k <= 9 else 0))
    random.seed(77)
    rows = DeviceRandAugment(4, 30).describe(10, (50, 70))
    assert [(o.name, o.sign) for r in rows for o in r] == picks
    # every magnitude of every bin count agrees with the restatement's table
    for bins, mag in [(31, 0), (31, 30), (11, 5), (2, 1)]:
        ra = DeviceRandAugment(1, mag, bins)
        for name in A.NAMES:
            for sign in (0, 1):
                o = ra.op(name, sign, 45, 61)
                assert (o.op, o.factor, tuple(o.args)) == tuple(A.policy_op(name, sign, mag, bins, 45, 61)), (bins, mag, name, sign)
    with pytest.raises(ValueError):
        DeviceRandAugment(5)
    with pytest.raises(ValueError):
        DeviceRandAugment(2, 31)
    with pytest.raises(ValueError):
        DeviceRandAugment(fill=(0, 0, 256))
    with pytest.raises(RuntimeError):
        DeviceRandAugment()(np.zeros((1, 3, 4, 4), dtype=np.uint8))  # no CPU path


def test_golden_chains_are_pillows_bytes_and_the_file_regenerates():
    pytest.importorskip("PIL")
    import make_randaug_golden as M
    g = np.load(G)
    src = g["src"]
    for (s, names), want in zip(M.CHAINS, g["chain_out"]):
        img = src[s]
        for name, sign, step in names:
            img = A.pil_policy_op(img, name, sign, step, M.BINS, M.FILL)
        assert np.array_equal(img, want), names
    fresh = M.build()
    assert sorted(fresh) == sorted(g.files)
    for k, v in fresh.items():
        v = np.asarray(v)
        assert v.dtype == g[k].dtype and v.shape == g[k].shape and v.tobytes() == g[k].tobytes(), k


def _item(ops=((2, 1.1, ()),), nops=None, reserved=0):
    from mnasnet_pytorch_amd import _lib as L
    it = L.MnasImgAug()
    it.nops = len(ops) if nops is None else nops
    for k, (op, f, args) in enumerate(ops):
        it.op[k], it.factor[k] = op, f
        for j, v in enumerate(args):
            it.arg[k][j] = v
    it.reserved = reserved
    return it


def test_host_check_refuses_every_bad_item():
    from mnasnet_pytorch_amd import _lib as L
    from mnasnet_pytorch_amd import augment as AU
    lib = L.load()
    assert ctypes.sizeof(L.MnasImgAug) == 136 and L.IMGA_MAX_OPS == A.MAX_OPS == 4
    assert (L.IMGA_IDENTITY, L.IMGA_AFFINE, L.IMGA_SHARPNESS, L.IMGA_INVERT, L.IMGA_EQUALIZE) == (A.IDENTITY, A.AFFINE, A.SHARPNESS,
                                                                                              A.INVERT, A.EQUALIZE)

    def check(items, n=None, h=24, w=40):
        arr = (L.MnasImgAug * max(1, len(items)))(*items)
        return lib.mnas_img_aug_check(arr, len(items) if n is None else n, h, w)

    shear = A.fixed_matrix((1, 0.3, 0, 0, 1, 0))
    good = [_item(), _item(ops=()), _item(ops=((A.AFFINE, 0.0, shear), (A.EQUALIZE, 0.0, ()), (A.AUTOCONTRAST, 0.0, ()), (A.CONTRAST, 0.0, ()))),
            _item(ops=((A.POSTERIZE, 0.0, (1,)), (A.POSTERIZE, 0.0, (8,)), (A.SOLARIZE, 0.0, (0,)), (A.SOLARIZE, 0.0, (256,)))),
            _item(ops=((A.AFFINE, 0.0, A.fixed_matrix((1, 0, -7, 0, 1, 300))), (A.INVERT, -1.0, ()), (A.IDENTITY, math.nan, ()))),
            _item(ops=((A.SHARPNESS, 1e30, ()),))]
    assert check(good) == 0 and check([]) == 0
    big = 1 << 30
    bad = [
        dict(nops=-1), dict(nops=5), dict(reserved=1), dict(reserved=-1),
        dict(ops=((-1, 1.0, ()),)), dict(ops=((11, 1.0, ()),)), dict(ops=((A.INVERT, 0.0, ()), (99, 0.0, ()))),      # unknown ops
        dict(ops=((A.BRIGHTNESS, -0.5, ()),)), dict(ops=((A.COLOR, math.inf, ()),)), dict(ops=((A.CONTRAST, math.nan, ()),)),
        dict(ops=((A.IDENTITY, 0.0, ()), (A.SHARPNESS, -1e-30, ()))),                # every factor k < nops is checked
        dict(ops=((A.POSTERIZE, 0.0, (0,)),)), dict(ops=((A.POSTERIZE, 0.0, (9,)),)),
        dict(ops=((A.SOLARIZE, 0.0, (-1,)),)), dict(ops=((A.SOLARIZE, 0.0, (257,)),)),
        dict(ops=((A.AFFINE, 0.0, (big, 1, 0, 0, 65536, 0)),)),                      # x a0 leaves int32 at x = W
        dict(ops=((A.AFFINE, 0.0, (65536, 1, 0, 7, -big, 0)),)),                     # y a4 leaves int32 at y = H
        dict(ops=((A.AFFINE, 0.0, (65536, 3, 2147483647, 0, 65536, 32768)),)),       # a2 + x a0 past 2^31
        dict(ops=((A.AFFINE, 0.0, (98304, 0, 32768, 0, 65536, 32768)),)),            # a1 == a3 == 0 with a scale
        dict(ops=((A.AFFINE, 0.0, (65536, 0, 65536, 0, 65536, 32768)),)),            # a1 == a3 == 0 with a fractional translation
        dict(ops=((A.AFFINE, 0.0, (0, 0, 0, 0, 0, 0)),)),
    ]
    for kw in bad:
        assert check([_item(**kw)]) == L.EINVAL, kw
        assert check([_item(), _item(**kw)]) == L.EINVAL, kw        # the bad one need not be first
    assert check([_item()], h=0) == L.EINVAL and check([_item()], w=0) == L.EINVAL
    assert check([_item()], h=16385) == L.EINVAL and check([_item()], w=16385) == L.EINVAL
    assert check([_item()], n=-1) == L.EINVAL and check([_item()], n=65536) == L.EINVAL
    assert lib.mnas_img_aug_check(None, 1, 24, 40) == L.EINVAL
    # workspace: a spare batch (16-byte rounded) from two ops on, 769 uint32 per (image, 16384-pixel chunk) with statistics
    assert lib.mnas_img_aug_workspace_bytes(256, 224, 224, 1, 0) == 0 and lib.mnas_img_aug_workspace_bytes(256, 224, 224, 0, 0) == 0
    assert lib.mnas_img_aug_workspace_bytes(256, 224, 224, 2, 0) == 256 * 3 * 224 * 224
    assert lib.mnas_img_aug_workspace_bytes(256, 224, 224, 1, 1) == 256 * 4 * 769 * 4
    assert lib.mnas_img_aug_workspace_bytes(3, 61, 83, 4, 1) == ((3 * 3 * 61 * 83 + 15) & ~15) + 3 * 769 * 4
    assert lib.mnas_img_aug_workspace_bytes(1, 0, 4, 1, 0) == -1 and lib.mnas_img_aug_workspace_bytes(1, 4, 4, 5, 0) == -1
    # the launch wrapper refuses before launching (n == 0 launches nothing): bad plan, fill, overlap, missing or unaligned workspace
    assert lib.mnas_img_aug(None, 0, 8, 8, 2, 0, 0, None, None, None, None) == 0
    assert lib.mnas_img_aug(16, 1, 8, 8, 5, 0, 0, 4096, 8192, None, None) == L.EINVAL
    assert lib.mnas_img_aug(16, 1, 8, 8, 1, 2, 0, 4096, 8192, 16384, None) == L.EINVAL         # a statistics stage past the last
    assert lib.mnas_img_aug(16, 1, 8, 8, 1, 0, 1 << 24, 4096, 8192, None, None) == L.EINVAL
    assert lib.mnas_img_aug(16, 1, 8, 8, 1, 0, 0, 4096, 4096 + 64, None, None) == L.EINVAL
    assert lib.mnas_img_aug(16, 1, 8, 8, 2, 0, 0, 4096, 8192, None, None) == L.EINVAL
    assert lib.mnas_img_aug(16, 1, 8, 8, 2, 0, 0, 4096, 8192, 16384 + 4, None) == L.EINVAL
    assert lib.mnas_img_aug(16, 1, 8, 8, 2, 0, 0, 4096, 8192, 8192 + 64, None) == L.EINVAL
    # descriptors from op lists, and the launch plan: chains are right-aligned, so a statistics op's stage depends on its chain's length
    rows = [[(A.EQUALIZE, 0.0, ())], [], [(A.AFFINE, 0.0, shear), (A.INVERT, 0.0, ()), (A.CONTRAST, 1.5, ())],
            [(A.AUTOCONTRAST, 0.0, ()), (A.SOLARIZE, 0.0, (128,))]]
    arr = AU.aug_items(rows)
    assert lib.mnas_img_aug_check(arr, 4, 24, 40) == 0
    assert [arr[k].nops for k in range(4)] == [1, 0, 3, 2] and list(arr[2].arg[0]) == list(shear) and arr[2].factor[2] == 1.5
    assert arr[3].arg[1][0] == 128 and arr[3].op[0] == A.AUTOCONTRAST
    assert AU.aug_plan(arr, 4) == (3, 0b110) and AU.aug_plan(arr, 2) == (1, 0b1) and AU.aug_plan(AU.aug_items([[], []]), 2) == (0, 0)
    with pytest.raises(ValueError):
        AU.aug_items([[(A.INVERT, 0.0, ())] * 5])
    assert AU.affine_args((1, 0.3, 0, 0, 1, 0)) == shear and AU.rotate_matrix(17.5, 33, 47) == A.rotate_matrix(17.5, 33, 47)
