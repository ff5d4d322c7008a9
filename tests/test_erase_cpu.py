"""CPU (no GPU needed): Random Erasing's host side.  Philox4x32-10's known answers against the numpy restatement and against a host
call of csrc/mnas_rng.h; the quantile table; mnas_img_erase_check on every legal edge and every field's violation; the struct's size;
DeviceRandomErasing.describe under a seed against the restatement of its documented draw order (tests/erase_ref.py)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import erase_ref as R


def _host_philox(lib, ctr, key):
    out = (ctypes.c_uint32 * 4)()
    lib.mnas_philox4x32_10((ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), out)
    return tuple(out)


def test_philox_known_answers():
    from mnasnet_pytorch_amd import _lib as L
    lib = L.load()
    for ctr, key, want in R.KNOWN:
        assert tuple(int(v) for v in R.philox(*ctr, *key)) == want
        assert _host_philox(lib, ctr, key) == want
    # the vectorised restatement and the header agree off the known answers as well, word for word
    rng = np.random.default_rng(5)
    ctrs = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    key = (0x01234567, 0x89abcdef)
    got = np.stack(R.philox(ctrs[:, 0], ctrs[:, 1], ctrs[:, 2], ctrs[:, 3], *key), axis=1)
    for row, ctr in zip(got, ctrs):
        assert tuple(int(v) for v in row) == _host_philox(lib, [int(v) for v in ctr], key)
    # every counter word and both key words reach the output
    base = tuple(int(v) for v in R.philox(1, 2, 3, 4, 5, 6))
    for k in range(6):
        arg = [1, 2, 3, 4, 5, 6]
        arg[k] += 1
        assert tuple(int(v) for v in R.philox(*arg)) != base


def test_table():
    from mnasnet_pytorch_amd import erase_table
    from mnasnet_pytorch_amd.erasing import IMAGENET_MEAN, IMAGENET_STD
    assert (IMAGENET_MEAN, IMAGENET_STD) == (R.IMAGENET_MEAN, R.IMAGENET_STD)
    t = erase_table()
    assert isinstance(t, bytes) and len(t) == 3 * 4096
    tab = np.frombuffer(t, dtype=np.uint8).reshape(3, 4096)
    assert np.array_equal(tab, R.table())
    clamps = []
    for c in range(3):
        assert bool((np.diff(tab[c].astype(np.int64)) >= 0).all())                                   # monotone
        assert tab[c, 2047] == tab[c, 2048] == int(round(255 * IMAGENET_MEAN[c]))                    # the median is the mean
        clamps.append((int((tab[c] == 0).sum()), int((tab[c] == 255).sum())))
    assert clamps == [(72, 51), (87, 32), (149, 17)]                                                 # bytes cannot hold the tails
    # other constants: std 0 is the mean's byte everywhere; the table follows mean and std
    flat = np.frombuffer(erase_table((0.5, 0.25, 1.0), (0.0, 0.0, 0.0)), dtype=np.uint8).reshape(3, 4096)
    assert [set(flat[c]) for c in range(3)] == [{128}, {64}, {255}]
    other = (0.4, 0.5, 0.6), (0.1, 0.3, 0.2)
    assert np.array_equal(np.frombuffer(erase_table(*other), dtype=np.uint8).reshape(3, 4096), R.table(*other))
    with pytest.raises(ValueError):
        erase_table((0.5, 0.5), (0.1, 0.1))
    with pytest.raises(ValueError):
        erase_table((0.5, 0.5, 0.5), (0.1, -0.1, 0.1))


def _item(L, mode=0, y0=0, x0=0, y1=0, x1=0, fill=(0, 0, 0), pad=0, reserved=(0, 0)):
    return L.MnasImgErase(mode, y0, x0, y1, x1, (ctypes.c_uint8 * 3)(*fill), pad, (ctypes.c_int32 * 2)(*reserved))


def test_struct_size_and_layout():
    from mnasnet_pytorch_amd import _lib as L
    assert ctypes.sizeof(L.MnasImgErase) == 32
    assert (L.IMGE_NONE, L.IMGE_CONST, L.IMGE_NOISE) == (R.NONE, R.CONST, R.NOISE) and L.IMGE_TABLE == R.TABLE
    E = L.MnasImgErase
    assert [getattr(E, f).offset for f in ("mode", "y0", "x0", "y1", "x1", "fill", "pad", "reserved")] == [0, 4, 8, 12, 16, 20, 23, 24]


def test_host_check_accepts_and_refuses():
    from mnasnet_pytorch_amd import _lib as L
    lib = L.load()
    n, H, W = 4, 6, 9

    def check(items, n_=n, h=H, w=W):
        arr = (L.MnasImgErase * max(1, len(items)))(*items)
        return lib.mnas_img_erase_check(arr, n_, h, w)

    ok = [_item(L), _item(L, 1, 0, 0, 6, 9, (1, 2, 3)), _item(L, 2, 0, 0, 6, 9), _item(L, 1, 6, 9, 6, 9), _item(L, 2, 2, 3, 2, 3),
          _item(L, 2, 2, 3, 2, 8), _item(L, 1, 2, 3, 5, 3), _item(L, 0, 1, 1, 5, 8, (255, 255, 255)), _item(L, 2, 5, 8, 6, 9)]
    for it in ok:                                                  # empty boxes, the full image, a corner pixel, any fill
        assert check([it] * n) == 0
    assert check([], 0) == 0 and lib.mnas_img_erase_check(None, 0, H, W) == 0
    for h, w in [(1, 9), (6, 1), (1, 1), (16384, 16384)]:          # H or W = 1, the largest image
        assert check([_item(L, 2, 0, 0, h, w), _item(L, 1, 0, 0, 1, 1), _item(L), _item(L, 1, h, w, h, w)], n, h, w) == 0
    assert check([ok[0]] * 3, 3) == 0
    arr = (L.MnasImgErase * 65535)()
    assert lib.mnas_img_erase_check(arr, 65535, H, W) == 0 and lib.mnas_img_erase_check(arr, 65536, H, W) == L.EINVAL
    bad = [_item(L, 3), _item(L, -1), _item(L, 1, 3, 0, 2, 0), _item(L, 1, 0, 5, 0, 4), _item(L, 1, -1, 0, 2, 2), _item(L, 1, 0, -1, 2, 2),
           _item(L, 1, 0, 0, 7, 2), _item(L, 1, 0, 0, 2, 10), _item(L, 1, 7, 0, 7, 0), _item(L, 1, 0, 10, 0, 10),
           _item(L, 0, pad=1), _item(L, 0, reserved=(1, 0)), _item(L, 0, reserved=(0, 1)),
           _item(L, 0, 0, 0, 7, 0)]                                # every field is checked whatever the mode
    for it in bad:
        assert check([it] * n) == L.EINVAL, bytes(it)
        assert check([ok[1], ok[2], it, ok[0]]) == L.EINVAL        # one refused item refuses the batch
    assert check([ok[0]] * n, n, 0, W) == L.EINVAL and check([ok[0]] * n, n, H, 0) == L.EINVAL
    assert check([ok[0]] * n, n, H, 16385) == L.EINVAL and check([ok[0]] * n, n, 16385, W) == L.EINVAL
    assert check([ok[0]], -1) == L.EINVAL
    assert lib.mnas_img_erase_check(None, 2, H, W) == L.EINVAL
    # the launch wrapper refuses a bad shape or a null pointer before it launches; n = 0 is nothing to do
    assert lib.mnas_img_erase(None, 1, 0, 4, None, None, 0, 0, None) == L.EINVAL
    assert lib.mnas_img_erase(None, 1, 4, 4, None, None, 0, 0, None) == L.EINVAL
    assert lib.mnas_img_erase(None, 0, 4, 4, None, None, 0, 0, None) == 0


CONFIGS = [dict(), dict(prob=1.0), dict(prob=1.0, mode="rand"), dict(prob=0.6, mode="const", value=(1, 2, 3)),
           dict(prob=0.8, mode="rand", min_count=1, max_count=4), dict(prob=1.0, min_count=3, max_area=0.9),
           dict(prob=1.0, min_area=0.5, max_area=0.99, min_aspect=0.1, max_aspect=0.5),
           dict(prob=0.5, mean=(0.4, 0.5, 0.6), std=(0.1, 0.3, 0.2), mode="rand")]


@pytest.mark.parametrize("kw", CONFIGS)
def test_describe_matches_restatement(kw):
    from mnasnet_pytorch_amd import DeviceRandomErasing
    er = DeviceRandomErasing(**kw)
    lo, hi = kw.get("min_count", 1), kw.get("max_count") or kw.get("min_count", 1)
    erased = total = 0
    for seed in range(10):
        for n, h, w in [(8, 64, 48), (5, 17, 33), (3, 224, 224), (4, 1, 1), (2, 2, 3), (0, 8, 8)]:
            random.seed(seed)
            got, got_seed = er.describe(n, h, w)
            after = random.random()
            random.seed(seed)
            want, want_seed = R.describe(n, h, w, **kw)
            assert after == random.random()                      # the same number of draws consumed
            assert [[tuple(b) for b in boxes] for boxes in got] == want and got_seed == want_seed
            assert len(got) == n and 0 <= got_seed < 1 << 64
            for boxes in got:
                total += 1
                erased += bool(boxes)
                assert len(boxes) <= hi
                for b in boxes:
                    y0, x0, y1, x1 = b.box
                    assert 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w and y1 - y0 < h and x1 - x0 < w
                    assert b.mode == (R.NOISE if er.mode == "pixel" else R.CONST)
                    if er.mode == "const":
                        assert b.fill == tuple(kw.get("value", (0, 0, 0)))
                    assert len(b.fill) == 3 and all(0 <= v <= 255 for v in b.fill)
                if h == 1 or w == 1:
                    assert boxes == []                           # a box must be smaller than the image on both sides
    assert lo >= 1 and 0 < erased <= total


def test_describe_prob_count_and_images_too_small():
    from mnasnet_pytorch_amd import DeviceRandomErasing
    random.seed(3)
    draws, _ = DeviceRandomErasing(prob=0.0).describe(50, 64, 64)
    assert draws == [[]] * 50
    draws, _ = DeviceRandomErasing(prob=1.0).describe(50, 64, 64)
    assert all(len(b) == 1 for b in draws)                       # default areas and aspects always fit a 64 x 64 image
    counts = set()
    for _ in range(20):
        draws, _ = DeviceRandomErasing(prob=1.0, min_count=2, max_count=5).describe(20, 96, 96)
        counts |= {len(b) for b in draws}
    assert counts == {2, 3, 4, 5}
    # an image no box fits: 10 attempts per box, every one as large as the image -> no box, mode NONE
    from mnasnet_pytorch_amd import _lib as L
    er = DeviceRandomErasing(prob=1.0, min_area=1.0, max_area=1.0, min_aspect=1.0, max_aspect=1.0)
    for h, w in [(2, 2), (7, 7), (1, 1)]:
        draws, _ = er.describe(3, h, w)
        assert draws == [[], [], []]
        assert all(it.mode == L.IMGE_NONE for it in DeviceRandomErasing.items(draws, 0))
    draws, _ = DeviceRandomErasing(prob=1.0, min_count=1, max_count=3).describe(6, 1, 1)
    assert draws == [[]] * 6
    for bad in (dict(prob=1.5), dict(min_area=0.0), dict(min_area=0.5, max_area=0.4), dict(min_aspect=0.0), dict(min_aspect=2.0, max_aspect=1.0),
                dict(mode="noise"), dict(value=(0, 0, 256)), dict(value=(0, 0)), dict(min_count=0), dict(min_count=3, max_count=2)):
        with pytest.raises(ValueError):
            DeviceRandomErasing(**bad)


def test_describe_items_round_trip_and_host_check():
    from mnasnet_pytorch_amd import DeviceRandomErasing
    from mnasnet_pytorch_amd import _lib as L
    lib = L.load()
    random.seed(11)
    er = DeviceRandomErasing(prob=0.7, mode="rand", min_count=1, max_count=3)
    n, h, w = 9, 40, 56
    draws, _ = er.describe(n, h, w)
    positions = max(len(b) for b in draws)
    assert positions >= 2
    back = [[] for _ in range(n)]
    for p in range(positions):
        arr = DeviceRandomErasing.items(draws, p)
        assert len(arr) == n and lib.mnas_img_erase_check(arr, n, h, w) == 0
        want = R.position_items([[tuple(b) for b in boxes] for boxes in draws], p)
        for k, it in enumerate(arr):
            assert (it.mode, (it.y0, it.x0, it.y1, it.x1), tuple(it.fill)) == want[k]
            assert it.pad == 0 and tuple(it.reserved) == (0, 0)
            if it.mode != L.IMGE_NONE:
                back[k].append((it.mode, (it.y0, it.x0, it.y1, it.x1), tuple(it.fill)))
    assert back == [[tuple(b) for b in boxes] for boxes in draws]
    assert all(it.mode == L.IMGE_NONE for it in DeviceRandomErasing.items(draws, positions))
    assert len(DeviceRandomErasing.items([], 0)) == 1            # ctypes has no empty array; n = 0 reads none of it


def test_reference_erase_rules():
    """the restatement against the header's sentences: absolute coordinates, positions and seeds, the later box wins"""
    tab = R.table()
    x = np.full((2, 3, 12, 21), 7, dtype=np.uint8)
    full = R.erase_position(x.copy(), [(R.NOISE, (0, 0, 12, 21), (0, 0, 0))] * 2, tab, 99, 0)
    part = R.erase_position(x.copy(), [(R.NOISE, (3, 5, 9, 18), (0, 0, 0))] * 2, tab, 99, 0)
    assert np.array_equal(part[:, :, 3:9, 5:18], full[:, :, 3:9, 5:18])          # the same pixel, the same byte, whichever box
    outside = np.ones_like(x, dtype=bool)
    outside[:, :, 3:9, 5:18] = False
    assert bool((part[outside] == 7).all())
    assert not np.array_equal(full[0], full[1]) and not np.array_equal(full[0, 0], full[0, 1])
    assert not np.array_equal(full, R.erase_position(x.copy(), [(R.NOISE, (0, 0, 12, 21), (0, 0, 0))] * 2, tab, 99, 1))
    assert not np.array_equal(full, R.erase_position(x.copy(), [(R.NOISE, (0, 0, 12, 21), (0, 0, 0))] * 2, tab, 100, 0))
    assert not np.array_equal(full, R.erase_position(x.copy(), [(R.NOISE, (0, 0, 12, 21), (0, 0, 0))] * 2, tab, 99 + (1 << 32), 0))
    # one pixel by hand
    n, c, y, xx, k, seed = 1, 2, 7, 13, 0, 99
    r = [int(v) for v in R.philox(xx >> 3, y, 3 * n + c, k, seed & 0xFFFFFFFF, seed >> 32)]
    word = r[(xx & 7) >> 1]
    half = word >> 16 if xx & 1 else word & 0xFFFF
    assert full[n, c, y, xx] == tab[c][half & 4095]
    draws = [[(R.CONST, (2, 2, 8, 10), (1, 2, 3)), (R.CONST, (5, 6, 11, 20), (4, 5, 6))], []]
    out = R.erase_batch(x, draws, tab, 0)
    assert bool((x == 7).all()) and bool((out[1] == 7).all())
    assert out[0, 0, 3, 3] == 1 and out[0, 2, 6, 7] == 6 and out[0, 1, 10, 19] == 5 and out[0, 0, 0, 0] == 7


def test_python_surface_refuses_cpu_tensors():
    import mnasnet_pytorch_amd as P
    for name in ("DeviceRandomErasing", "erase_table"):
        assert name in P.__all__ and hasattr(P, name)
    x = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    er = P.DeviceRandomErasing()
    with pytest.raises(RuntimeError):
        er(x)
    with pytest.raises(RuntimeError):
        er.apply(x, [[], []], 0)
