"""CPU (no GPU needed): the image batch transform's host half.  The numpy restatement (tests/img_xform_ref.py) is Pillow's crop +
BILINEAR resize bit for bit; DeviceTransform.from_reference draws the reference's geometry (datasets.py preprocess_img);
get_params keeps RandomResizedCrop's properties; mnas_img_xform_check refuses every kind of bad descriptor (host function
only: nothing here launches a kernel); collate_decoded batches decoded images of mixed sizes from ClusterRandomSampler."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import cases as C
import img_xform_ref as R

G = os.path.join(C.GOLDEN_DIR, "img_xform.npz")


def _random_case(rng):
    h, w = int(rng.integers(1, 400)), int(rng.integers(1, 400))
    c = int(rng.choice([1, 3, 4]))
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    bh, bw = int(rng.integers(1, h + 1)), int(rng.integers(1, w + 1))
    box = (int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1)), bh, bw)
    rh = int(rng.integers(max(1, -(-bh // 32)), 500))
    rw = int(rng.integers(max(1, -(-bw // 32)), 500))
    ho, wo = int(rng.integers(1, rh + 1)), int(rng.integers(1, rw + 1))
    win = (int(rng.integers(0, rh - ho + 1)), int(rng.integers(0, rw - wo + 1)))
    return img, box, (rh, rw), win, (ho, wo), int(rng.integers(0, 4))


def test_restatement_matches_pillow_random():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(2026)
    for _ in range(120):
        args = _random_case(rng)
        assert np.array_equal(R.xform(*args), R.pil_xform(*args)), args[1:]
    # the sizes a training run meets: a 2000 x 1500 photo to 224^2, 375 x 500 to 512 x 384, and a 30x strip
    for (h, w), (ho, wo) in [((1500, 2000), (224, 224)), ((375, 500), (384, 512)), ((97, 3000), (5, 100))]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        args = (img, (0, 0, h, w), (ho, wo), (0, 0), (ho, wo), 1)
        assert np.array_equal(R.xform(*args), R.pil_xform(*args)), (h, w, ho, wo)


def _golden_sources(g):
    buf = g["src"]
    return [buf[o:o + h * w * c].reshape(h, w, c) for o, h, w, c in g["src_meta"]]


def test_restatement_matches_golden():
    g = np.load(G)
    srcs = _golden_sources(g)
    for k, row in enumerate(g["cases"]):
        s, bt, bl, bh, bw, rh, rw, wt, wl, f, ho, wo = (int(v) for v in row)
        got = R.xform(srcs[s], (bt, bl, bh, bw), (rh, rw), (wt, wl), (ho, wo), f)
        o = int(g["out_off"][k])
        assert np.array_equal(got.reshape(-1), g["out"][o:o + got.size]), k
    for row, want in zip(g["e2e_cases"], g["e2e_out"]):
        s, bt, bl, bh, bw, rh, rw, wt, wl, f, ho, wo = (int(v) for v in row)
        assert np.array_equal(R.xform(srcs[s], (bt, bl, bh, bw), (rh, rw), (wt, wl), (ho, wo), f), want)
    # every stored case is one the device accepts (the GPU test launches them all)
    from mnasnet_pytorch_amd import _lib as L
    lib = L.load()
    for row in list(g["cases"]) + list(g["e2e_cases"]):
        s, bt, bl, bh, bw, rh, rw, wt, wl, f, ho, wo = (int(v) for v in row)
        o, h, w, c = (int(v) for v in g["src_meta"][s])
        it = L.MnasImgXform(o, h, w, c, w * c, bt, bl, bh, bw, rh, rw, wt, wl, f, 0)
        assert lib.mnas_img_xform_check(ctypes.byref(it), 1, ho, wo, g["src"].size) == 0, row


def test_from_reference_geometry():
    from mnasnet_pytorch_amd.transforms import DeviceTransform as T
    shapes = [(300, 400, 3), (400, 300, 1), (224, 225, 4), (224, 224, 3)]
    # 0: Resize(fixed_size) -- also the validation transform
    hw, d = T.from_reference(0, fixed_size=(224, 256)).describe(shapes)
    assert hw == (224, 256) and d[0] == (0, 0, 300, 400, 224, 256, 0, 0, 0) and d[1] == (0, 0, 400, 300, 224, 256, 0, 0, 0)
    # 1: Resize(s) + CenterCrop(fixed_size): shorter side -> s, longer int(s * long / short), window int(round((r - t) / 2.))
    hw, d = T.from_reference(1).describe(shapes)
    assert hw == (224, 224)
    assert d[0] == (0, 0, 300, 400, 224, int(224 * 400 / 300), 0, int(round((298 - 224) / 2.)), 0) == (0, 0, 300, 400, 224, 298, 0, 37, 0)
    assert d[1] == (0, 0, 400, 300, 298, 224, 37, 0, 0)
    assert d[2] == (0, 0, 224, 225, 224, 225, 0, 0, 0)          # shorter side already s: unchanged; round(0.5) == 0 (Python 3)
    assert d[3] == (0, 0, 224, 224, 224, 224, 0, 0, 0)
    with pytest.raises(ValueError):                               # a centre crop wider than the resized image
        T.from_reference(1, fixed_size=(224, 320)).describe([(224, 224, 3)])
    # 2: Resize(final_size), final_size = cluster size x size_ratio (ProgressiveResize.cluster_shapes)
    from mnasnet_pytorch_amd.sampler import ProgressiveResize
    fs = ProgressiveResize(0.25, 256, 10).cluster_shapes()[0]
    hw, d = T.from_reference(2, final_size=fs).describe(shapes)
    assert hw == (96, 128) and all(x[:4] == (0, 0) + s[:2] and x[4:] == (96, 128, 0, 0, 0) for x, s in zip(d, shapes))
    hw, _ = T.from_reference(2).describe(shapes, target_size=(128, 96))      # per batch from ImageBatch.target_size
    assert hw == (128, 96)
    with pytest.raises(ValueError):
        T.from_reference(2).describe(shapes)
    # 4 / 5 / 6: RandomResizedCropRect(size[, scale, ratio]) + RandomHorizontalFlip()
    for typ, kw, size, scale, ratio in [(4, {"final_size": (96, 128)}, (96, 128), (0.08, 1.0), (3 / 4, 4 / 3)),
                                        (5, {}, (224, 224), (0.08, 1.0), (3 / 4, 4 / 3)),
                                        (6, {}, (224, 224), (0.7, 1.0), (0.7, 1.2))]:
        t = T.from_reference(typ, **kw)
        assert (t.mode, t.scale, t.ratio, t.hflip, t.vflip) == ("random_resized_crop", scale, ratio, 0.5, 0.0)
        random.seed(typ)
        hw, d = t.describe([(375, 500, 3)] * 400)
        assert hw == size
        assert all(x[4:8] == size + (0, 0) and x[8] in (0, 1) for x in d)
        assert 150 < sum(x[8] for x in d) < 250                  # p = 0.5 horizontal flips, never a vertical one
    for bad in (3, 7):
        with pytest.raises(ValueError):
            T.from_reference(bad)


def test_get_params_properties():
    from mnasnet_pytorch_amd.transforms import get_params
    random.seed(7)
    for scale, ratio in [((0.08, 1.0), (3 / 4, 4 / 3)), ((0.7, 1.0), (0.7, 1.2))]:
        for h, w in [(375, 500), (500, 375), (224, 224), (1500, 2000), (120, 90)]:
            for _ in range(300):
                i, j, ch, cw = get_params(h, w, scale, ratio)
                assert 0 <= i and 0 <= j and 1 <= ch and 1 <= cw and i + ch <= h and j + cw <= w
                s = min(h, w)
                if (i, j, ch, cw) == ((h - s) // 2, (w - s) // 2, s, s):
                    continue                                      # the centred-square fallback
                a = ch * cw / (h * w)
                r = max(cw / ch, ch / cw)                         # the coin flip swaps the sides
                tol = 1.0 / min(ch, cw)                           # sides are rounded to whole pixels
                assert scale[0] * (1 - 2 * tol) <= a <= scale[1] * (1 + 2 * tol), (h, w, ch, cw)
                assert 1 / max(ratio[1], 1 / ratio[0]) <= r * (1 + 2 * tol) and r <= max(ratio[1], 1 / ratio[0]) * (1 + 2 * tol)
    # nothing fits a 1000 x 10 strip at these ratios: the centred square
    random.seed(0)
    assert get_params(10, 1000) == (0, 495, 10, 10)
    # same seed, same descriptors (module-level random, as sampler.py)
    from mnasnet_pytorch_amd.transforms import DeviceTransform
    t = DeviceTransform.from_reference(4, final_size=(224, 224))
    shapes = [(375, 500, 3), (500, 333, 1), (64, 2000, 4)] * 20
    random.seed(11)
    a = t.describe(shapes)
    random.seed(11)
    assert t.describe(shapes) == a
    random.seed(12)
    assert t.describe(shapes) != a


def _item(**kw):
    from mnasnet_pytorch_amd import _lib as L
    d = dict(src_offset=32, src_h=40, src_w=50, src_c=3, src_stride=150, box_top=5, box_left=6, box_h=30, box_w=40, rh=20,
             rw=25, win_top=2, win_left=3, flags=3, reserved=0)
    d.update(kw)
    return L.MnasImgXform(**d)


def test_host_check_refuses_every_bad_item():
    from mnasnet_pytorch_amd import _lib as L
    lib = L.load()
    assert ctypes.sizeof(L.MnasImgXform) == 64
    src_bytes = 32 + 40 * 150 + 16 * 10                    # image at offset 32, room behind it
    ho, wo = 16, 20

    def check(items, n=None, h=ho, w=wo, nbytes=src_bytes):
        arr = (L.MnasImgXform * max(1, len(items)))(*items)
        return lib.mnas_img_xform_check(arr, len(items) if n is None else n, h, w, nbytes)

    assert check([_item()]) == 0 and check([_item(), _item(src_c=1, src_stride=50)]) == 0
    assert check([_item(src_c=4, src_stride=200)]) == L.EINVAL                  # 4 channels: the last row ends past src_bytes
    assert check([_item(src_c=4, src_stride=200)], nbytes=32 + 40 * 200) == 0
    assert check([]) == 0
    assert check([_item(box_h=640, box_w=800, src_h=700, src_w=900, src_stride=2700, box_top=0, box_left=0)],
                 nbytes=32 + 700 * 2700 + 16 * 4) == 0          # exactly 32x down on both axes: supported
    bad = [
        dict(src_c=2), dict(src_c=0), dict(src_c=5),                                     # channels
        dict(src_h=0), dict(src_w=0), dict(src_stride=149), dict(src_offset=-16),        # image geometry
        dict(src_offset=32 + 16 * 11),                                                   # image bytes past src_bytes
        dict(src_h=42),                                                                  # last row past src_bytes
        dict(box_top=-1), dict(box_left=-1), dict(box_h=0), dict(box_w=0),               # box
        dict(box_top=11), dict(box_left=11), dict(box_h=36), dict(box_w=45),             # box past the image
        dict(rh=0), dict(rw=0), dict(rh=17, win_top=2), dict(rw=22, win_left=3),         # window past the resized box
        dict(win_top=-1), dict(win_left=-1),
        dict(box_h=33, box_top=0, rh=1, win_top=0),                                     # more than 32x down
        dict(box_w=50, box_left=0, rw=1, win_left=0),
        dict(rh=65537), dict(rw=65537),
        dict(flags=4), dict(flags=-1), dict(reserved=1),
    ]
    for kw in bad:
        assert check([_item(**kw)]) == L.EINVAL, kw
        assert check([_item(), _item(**kw)]) == L.EINVAL, kw          # the bad one need not be first
    # batch-wide arguments
    assert check([_item()], h=0) == L.EINVAL and check([_item()], w=0) == L.EINVAL
    assert check([_item()], h=16385, w=20) == L.EINVAL
    assert check([_item()], nbytes=src_bytes + 8) == L.EINVAL          # src_bytes a multiple of 16
    assert check([_item()], n=-1) == L.EINVAL and check([_item()], n=65536) == L.EINVAL
    assert lib.mnas_img_xform_check(None, 1, ho, wo, src_bytes) == L.EINVAL


class _Decoded(torch.utils.data.Dataset):
    """a dataset the way INTEGRATION.md section 4 wires the reference's: (decoded HWC uint8, target, cluster target size)"""
    SIZES = {0: (96, 128), 1: (128, 128), 2: (128, 96)}

    def __init__(self):
        rng = np.random.default_rng(3)
        self.items, self.cluster_indices = [], [[], [], []]
        for i in range(60):
            k = i % 3
            h, w = int(rng.integers(20, 90)), int(rng.integers(20, 90))
            c = [1, 3, 4][i % 3]
            img = rng.integers(0, 256, (h, w) if c == 1 and i % 2 else (h, w, c), dtype=np.uint8)
            self.items.append((img, i % 10, self.SIZES[k]))
            self.cluster_indices[k].append(i)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_collate_decoded_with_cluster_sampler():
    from mnasnet_pytorch_amd import ClusterRandomSampler, ImageBatch, collate_decoded
    ds = _Decoded()
    random.seed(5)
    loader = torch.utils.data.DataLoader(ds, batch_size=8, sampler=ClusterRandomSampler(ds, 8), collate_fn=collate_decoded)
    seen = 0
    for batch, target in loader:
        assert isinstance(batch, ImageBatch) and len(batch) == 8 and target.shape == (8,)
        assert batch.data.numel() % 16 == 0 and batch.target_size in _Decoded.SIZES.values()
        assert len({s[:2] for s in batch.shapes}) > 1                    # mixed source sizes in one batch
        end = 0
        for i in range(8):
            h, w, c = batch.shapes[i]
            assert batch.offsets[i] == end                               # back to back
            end += h * w * c
            img = batch.image(i)
            # identify the sample: same pixels, same target, same cluster size
            match = [k for k, (a, t, sz) in enumerate(ds.items)
                     if a.shape[:2] == (h, w) and np.array_equal(a.reshape(h, w, -1), img)]
            assert len(match) == 1 and ds.items[match[0]][1] == int(target[i])
            assert ds.items[match[0]][2] == batch.target_size
        seen += 8
    assert seen == 48                                                    # 3 clusters x 20 images: two full batches each
    with pytest.raises(ValueError):
        collate_decoded([ds[0], ds[1]])                                  # two clusters' sizes in one batch
    b, t = collate_decoded([(np.zeros((3, 5, 3), np.uint8), 1)])
    assert b.target_size is None and b.shapes == [(3, 5, 3)] and b.data.numel() == 48 and int(t[0]) == 1
