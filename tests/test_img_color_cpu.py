"""CPU (no GPU needed): the photometric image ops' host half.  The numpy restatement (tests/img_color_ref.py) is Pillow's
arithmetic over each function's whole input domain (all 2^24 RGB triples; all 65 536 blend pairs at 200+ factors); the type-3
restatement plus DevicePipeline.describe equals the literal Pillow Compose byte for byte and consumes the same draws;
DevicePipeline delegates types 0-2 and 4-6 to DeviceTransform; mnas_img_color_check refuses every kind of bad item (host
function only: nothing here launches a kernel)."""
import ctypes
import itertools
import math
import random

import numpy as np
import pytest

import img_color_ref as R
import img_xform_ref as X


@pytest.fixture(scope="module")
def cube():
    pytest.importorskip("PIL")
    from PIL import Image
    img = R.cube_image()
    return img, Image.fromarray(img, "RGB"), R.CubeTables()


def test_grey_and_hsv_over_the_rgb_cube(cube):
    from PIL import Image
    img, im, tab = cube
    assert np.array_equal(R.grey(img[..., 0], img[..., 1], img[..., 2]), np.asarray(im.convert("L")))
    assert np.array_equal(tab.hsv.reshape(4096, 4096, 3), np.asarray(im.convert("HSV")))          # RGB -> HSV, every triple
    assert np.array_equal(tab.rgb.reshape(4096, 4096, 3), np.asarray(Image.fromarray(img, "HSV").convert("RGB")))  # HSV -> RGB
    # the direct restatement equals the tables (what the GPU tests use) on a sample
    idx = np.random.default_rng(0).integers(0, 1 << 24, 1 << 16)
    s = img.reshape(-1, 3)[idx]
    assert np.array_equal(np.stack(R.rgb_to_hsv(s[:, 0], s[:, 1], s[:, 2]), -1), tab.hsv[idx])
    assert np.array_equal(R.hue(s, 77), tab.hue(s, 77))


def test_hue_over_the_rgb_cube(cube):
    from mnasnet_pytorch_amd.transforms import hue_shift
    img, _, tab = cube
    # 0.2.x shifts of factors -0.5, -0.1, -1/255 (wrapped negative), 0.004, 0.1, 0.5
    assert [hue_shift(f) for f in (-0.5, -0.1, -1 / 255, 0.004, 0.1, 0.5)] == [129, 231, 255, 1, 25, 127]
    assert hue_shift(-0.1) == R.hue_shift(-0.1) == (np.int64(-25) % 256)
    for shift in (255, 231, 1):
        assert np.array_equal(tab.hue(img, shift), R.pil_op(img, R.HUE, shift=shift)), shift


def test_blend_all_pairs():
    pytest.importorskip("PIL")
    from PIL import Image
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    ia, ib = Image.fromarray(np.ascontiguousarray(a), "L"), Image.fromarray(np.ascontiguousarray(b), "L")
    factors = sorted(set([float(f) for f in np.linspace(0.0, 2.0, 201)] + [0.9, 1.1, 0.999999, 1.000001, 3.5, 40.0]))
    assert sum(f < 1 for f in factors) >= 100 and sum(f > 1 for f in factors) >= 100
    for f in factors:
        assert np.array_equal(R.blend(a, b, f), np.asarray(Image.blend(ia, ib, f))), f


def test_enhance_degenerates():
    """Brightness (0), Color (the pixel's L) and Contrast (the image's rounded mean) against ImageEnhance"""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(1)
    for h, w in [(37, 53), (64, 64)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for op in (R.BRIGHTNESS, R.SATURATION, R.CONTRAST):
            for f in (0.0, 0.5, 0.9, 0.95, 1.0, 1.05, 1.1, 1.7, 6.0):
                assert np.array_equal(R.apply_op(img, op, f), R.pil_op(img, op, f)), (op, f)


def test_contrast_mean_against_imagestat():
    pytest.importorskip("PIL")
    from PIL import Image, ImageStat
    rng = np.random.default_rng(2)
    n = 0
    for h, w in [(1, 2), (2, 3), (3, 3), (5, 7), (16, 16), (31, 17)]:
        for _ in range(40):
            # grey pixels (L = value): sums that land on k + 0.5 and one step either side
            L = rng.integers(0, 256, h * w)
            target = int(L.sum()) - int(L.sum()) % (h * w) + (h * w) // 2 + int(rng.integers(-1, 2))
            L[0] = np.clip(L[0] + target - int(L.sum()), 0, 255)
            img = np.repeat(L.reshape(h, w, 1), 3, axis=2).astype(np.uint8)
            want = int(ImageStat.Stat(Image.fromarray(img, "RGB").convert("L")).mean[0] + 0.5)
            assert R.contrast_mean(img) == want
            n += (2 * int(L.sum())) % (h * w) == 0 and (h * w) % 2 == 0
    assert n > 10                                                   # exact .5 means were met
    img = rng.integers(0, 256, (120, 90, 3), dtype=np.uint8)
    assert R.contrast_mean(img) == int(ImageStat.Stat(Image.fromarray(img, "RGB").convert("L")).mean[0] + 0.5)


def test_all_24_orders_against_pillow():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (29, 41, 3), dtype=np.uint8)
    for p in itertools.permutations([R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE]):
        fac = [float(v) for v in rng.uniform(0.85, 1.15, 4)]
        hf = float(rng.uniform(-0.1, 0.1))
        ops = [(op, hf if op == R.HUE else f) for op, f in zip(p, fac)]
        want = img
        for op, f in ops:
            want = R.pil_op(want, op, f, R.hue_shift(f) if op == R.HUE else 0)
        assert np.array_equal(R.jitter(img, ops), want), ops
        assert np.array_equal(R.color(img, list(p), [0.0 if op == R.HUE else f for op, f in ops], R.hue_shift(hf)), want)


def _sources(rng, n):
    out = []
    for k in range(n):
        h, w, c = int(rng.integers(20, 90)), int(rng.integers(20, 90)), int(rng.choice([1, 3, 4]))
        out.append(rng.integers(0, 256, (h, w) if c == 1 and k % 2 else (h, w, c), dtype=np.uint8))
    return out


def test_type3_compose_against_pillow():
    """the literal Pillow Compose of type 3 and DevicePipeline.describe + the numpy restatement: same bytes, same draws"""
    pytest.importorskip("PIL")
    from mnasnet_pytorch_amd import DevicePipeline
    rng = np.random.default_rng(4)
    for prob, size, seed in [(0.2, (40, 52), 1), (0.5, (33, 47), 2), (1.0, (48, 36), 3)]:
        imgs = _sources(rng, 16)
        random.seed(seed)
        pil = [R.pil_type3(a, size, prob) for a in imgs]
        after_pil = random.random()
        random.seed(seed)
        hw, draws = DevicePipeline.from_reference(3, final_size=size, prob=prob).describe([np.shape(a) for a in imgs])
        assert random.random() == after_pil                         # the same number of draws
        assert hw == size
        for a, want, d in zip(imgs, pil, draws):
            assert np.array_equal(R.type3(a, size, d), want), (prob, d)
        if prob == 1.0:
            assert all(d.applied and len(d.jitter) == 4 for d in draws)
    # prob 0: still one draw for RandomApply and each flip / grayscale, nothing applied
    random.seed(9)
    hw, draws = DevicePipeline.from_reference(3, final_size=(8, 8), prob=0.0).describe([(10, 10, 3)] * 5)
    random.seed(9)
    for _ in range(20):                                             # four draws per image
        random.random()
    x = random.random()
    random.seed(9)
    DevicePipeline.from_reference(3, final_size=(8, 8), prob=0.0).describe([(10, 10, 3)] * 5)
    assert random.random() == x
    assert all(d == (False, None, None, 0, False) for d in draws)


def test_type3_draws_reproducible_and_in_range():
    from mnasnet_pytorch_amd import DeviceColorJitter, DevicePipeline, DeviceRandomGrayscale
    from mnasnet_pytorch_amd import _lib as L
    pipe = DevicePipeline.from_reference(3, prob=0.5)
    shapes = [(375, 500, 3), (64, 2000, 1)] * 50
    random.seed(11)
    a = pipe.describe(shapes, target_size=(384, 512))
    random.seed(11)
    assert pipe.describe(shapes, target_size=(384, 512)) == a
    random.seed(12)
    assert pipe.describe(shapes, target_size=(384, 512)) != a
    for d in a[1]:
        if d.applied:
            assert sorted(op for op, _ in d.jitter) == [1, 2, 3, 4]
            assert all((-0.1 <= f <= 0.1) if op == L.IMGC_HUE else (0.9 <= f <= 1.1) for op, f in d.jitter)
            t, l, h, w = d.box
            assert 0 <= t and 0 <= l and t + h <= 384 and l + w <= 512
    orders = {tuple(op for op, _ in d.jitter) for d in a[1] if d.applied}
    assert len(orders) > 8                                          # the shuffle varies
    with pytest.raises(ValueError):
        pipe.describe(shapes)                                       # no final size
    # ColorJitter draws only the parameters > 0, in [B, C, S, H] order before the shuffle
    random.seed(3)
    d = DeviceColorJitter(0.0, 0.2, 0.0, 0.05).describe(200)
    assert all(sorted(op for op, _ in x) == [L.IMGC_CONTRAST, L.IMGC_HUE] for x in d)
    random.seed(3)
    c = random.uniform(0.8, 1.2)
    h = random.uniform(-0.05, 0.05)
    assert sorted(d[0]) == sorted([(L.IMGC_CONTRAST, c), (L.IMGC_HUE, h)])
    assert DeviceColorJitter().describe(3) == [[], [], []]
    random.seed(4)
    g = DeviceRandomGrayscale(0.3).describe(1000)
    assert 200 < sum(g) < 400
    with pytest.raises(ValueError):
        DeviceColorJitter(hue=0.6)


def test_delegation_to_device_transform():
    from mnasnet_pytorch_amd import DevicePipeline, DeviceTransform
    shapes = [(300, 400, 3), (400, 300, 1), (224, 225, 4)] * 10
    for typ in (0, 1, 2, 4, 5, 6):
        kw = {"final_size": (96, 128)} if typ in (2, 4) else {}
        random.seed(typ)
        a = DevicePipeline.from_reference(typ, prob=0.7, **kw).describe(shapes)
        ra = random.random()
        random.seed(typ)
        b = DeviceTransform.from_reference(typ, **kw).describe(shapes)
        assert a == b and random.random() == ra, typ
    with pytest.raises(ValueError):
        DeviceTransform.from_reference(3)
    with pytest.raises(ValueError):
        DevicePipeline.from_reference(7)


def test_same_size_resample_is_identity():
    """a same-size bilinear resample (taps [2^22, 0]) copies the image, as Pillow's resize does"""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(5)
    for h, w in [(1, 1), (2, 7), (37, 61), (224, 224), (96, 128)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        got = X.xform(img, (0, 0, h, w), (h, w), (0, 0), (h, w))
        assert np.array_equal(got, img.transpose(2, 0, 1))
        assert np.array_equal(got, X.pil_xform(img, (0, 0, h, w), (h, w), (0, 0), (h, w)))
        xmin, xmax, kk = X.coeffs(w, w)
        assert (kk[:, 0] == 1 << 22).all() and (kk[:, 1:] == 0).all() and (xmin == np.arange(w)).all()


def _item(**kw):
    from mnasnet_pytorch_amd import _lib as L
    it = L.MnasImgColor()
    it.nops = kw.pop("nops", 2)
    ops = kw.pop("ops", [L.IMGC_CONTRAST, L.IMGC_HUE])
    fac = kw.pop("factor", [1.05, 0.0])
    for j, (o, f) in enumerate(zip(ops, fac)):
        it.op[j], it.factor[j] = o, f
    it.hue_shift = kw.pop("hue_shift", 17)
    it.reserved = kw.pop("reserved", 0)
    assert not kw
    return it


def test_host_check_refuses_every_bad_item():
    from mnasnet_pytorch_amd import _lib as L
    lib = L.load()
    assert ctypes.sizeof(L.MnasImgColor) == 52

    def check(items, n=None, h=24, w=40):
        arr = (L.MnasImgColor * max(1, len(items)))(*items)
        return lib.mnas_img_color_check(arr, len(items) if n is None else n, h, w)

    assert check([_item()]) == 0 and check([]) == 0 and check([_item(nops=0)]) == 0
    assert check([_item(nops=5, ops=[1, 2, 3, 4, 5], factor=[0.0, 1e30, 2.0, 0.0, 0.0])]) == 0
    assert check([_item(nops=2, ops=[5, 5], factor=[0.0, 0.0], hue_shift=255)]) == 0
    bad = [
        dict(nops=-1), dict(nops=6),
        dict(ops=[0, 4]), dict(ops=[6, 4]), dict(ops=[2, -3]),                      # unknown ops
        dict(ops=[2, 2], factor=[1.0, 1.0]),                                        # two CONTRASTs
        dict(factor=[-0.5, 0.0]), dict(factor=[-1e-30, 0.0]), dict(factor=[math.inf, 0.0]), dict(factor=[math.nan, 0.0]),
        dict(factor=[1.0, -2.0]),                                                   # every factor k < nops is checked
        dict(hue_shift=-1), dict(hue_shift=256), dict(reserved=1), dict(reserved=-1),
    ]
    for kw in bad:
        assert check([_item(**kw)]) == L.EINVAL, kw
        assert check([_item(), _item(**kw)]) == L.EINVAL, kw        # the bad one need not be first
    assert check([_item()], h=0) == L.EINVAL and check([_item()], w=0) == L.EINVAL
    assert check([_item()], h=16385) == L.EINVAL and check([_item()], w=16385) == L.EINVAL
    assert check([_item()], n=-1) == L.EINVAL and check([_item()], n=65536) == L.EINVAL
    assert lib.mnas_img_color_check(None, 1, 24, 40) == L.EINVAL
    assert lib.mnas_img_color_workspace_bytes(256, 512, 384) == 256 * 12 * 4
    assert lib.mnas_img_color_workspace_bytes(1, 4096, 4096) == 1024 * 4 and lib.mnas_img_color_workspace_bytes(1, 0, 4) == -1
    # the launch wrapper refuses before launching: bad layout, partial overlap (n == 0 launches nothing)
    assert lib.mnas_img_color(None, 0, 8, 8, 0, None, 1, None, None, None) == 0
    assert lib.mnas_img_color(None, 1, 8, 8, 2, 16, 0, 4096, None, None) == L.EINVAL
    assert lib.mnas_img_color(16, 1, 8, 8, 0, 4096, 0, 4096 + 64, None, None) == L.EINVAL
    assert lib.mnas_img_color(16, 1, 8, 8, 0, 4096, 1, 4096, None, None) == L.EINVAL
