"""-m gpu: Random Erasing on the MI355X.  The erase kernel (csrc/mnas_imge.hip) through the C ABI, in place on a batch that sits
between 4096 canary bytes on each side, the WHOLE buffer compared byte for byte with the numpy restatement (tests/erase_ref.py)
applied to the same bytes on the host; DeviceRandomErasing under a seed against the restatement's draws; one Trainer step on a
batch erased on the device against the same step on the batch the restatement erased on the host (bit-equal)."""
import random

import numpy as np
import pytest
import torch

import erase_ref as R
from mnasnet_pytorch_amd import _lib as L

pytestmark = pytest.mark.gpu
PAD = 4096                                     # canary bytes on each side of the batch
CANARY = 0x5A
NO_BOX = (R.NONE, (0, 0, 0, 0), (0, 0, 0))
SEED = 0x9E3779B97F4A7C15                      # both key words in use

_state = {}


def _table():
    """the ImageNet table on the host (3, 4096) and on the device, built once and left unchanged"""
    if not _state:
        from mnasnet_pytorch_amd import erase_table
        _state["host"] = R.table()
        assert _state["host"].tobytes() == erase_table()
        _state["dev"] = torch.from_numpy(_state["host"].reshape(-1).copy()).cuda()
    return _state["host"], _state["dev"]


def _arr(items):
    from mnasnet_pytorch_amd.erasing import DeviceRandomErasing, EraseBox
    return DeviceRandomErasing.items([[] if it[0] == R.NONE else [EraseBox(*it)] for it in items], 0)


def _launch(buf, off, shape, arr, seed, position, table):
    n, _, h, w = shape
    items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
    L.check(L.load().mnas_img_erase(items.data_ptr(), n, h, w, buf.data_ptr() + PAD + off, L.ptr(table), seed, position, L.cur_stream()))


def _run(x, launches, off=0, seed=SEED, table="dev"):
    """x: host batch; launches: [(items, position)] run in order, in place, on x inside canary bytes at byte offset `off` of an
    aligned buffer -> the erased batch on the host, after the WHOLE buffer was compared with the restatement's"""
    host_tab, dev_tab = _table()
    size = x.size
    want = np.full(size + 2 * PAD + 64, CANARY, dtype=np.uint8)
    want[PAD + off:PAD + off + size] = x.reshape(-1)
    buf = torch.from_numpy(want.copy()).cuda()
    assert buf.data_ptr() % 16 == 0
    ref = x.copy()
    for items, position in launches:
        _launch(buf, off, x.shape, _arr(items), seed, position, dev_tab if table == "dev" else table)
        R.erase_position(ref, items, host_tab, seed, position)
    want[PAD + off:PAD + off + size] = ref.reshape(-1)
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%d bytes differ, first at buffer offset %d (batch starts at %d, %d bytes): got %d want %d; launches %r"
                             % (bad.size, bad[0], PAD + off, size, got[bad[0]], want[bad[0]], launches))
    return got[PAD + off:PAD + off + size].reshape(x.shape)


def _boxes(h, w):
    """the boxes every shape runs, clipped to the image: the full image, a pixel at each corner, widths 15 / 16 / 17 at x0 = 0 / 1 /
    15 / 16, boxes that end at the right edge, empty boxes, a box whose x0 and x1 are not multiples of 8"""
    out = [(0, 0, h, w), (0, 0, 1, 1), (0, w - 1, 1, w), (h - 1, 0, h, 1), (h - 1, w - 1, h, w)]
    y0, y1 = h // 3, max(h // 3 + 1, h - h // 4)
    for x0 in (0, 1, 15, 16):
        for width in (15, 16, 17):
            if x0 < w:
                out.append((y0, x0, y1, min(x0 + width, w)))
    out += [(y0, w // 2, y1, w), (0, max(w - 17, 0), h, w), (h - 1, max(w - 3, 0), h, w)]              # flush with the right edge
    out += [(0, 0, 0, 0), (h, w, h, w), (y0, w // 2, y0, w), (y0, w // 2, y1, w // 2)]                  # empty
    if w >= 6:
        out.append((y0, 3, y1, (w - 5) // 8 * 8 + 5))                                                   # x0 = 3, x1 = 5 mod 8
    if w >= 11:
        out.append((min(1, h - 1), 9, h, min(w, 43)))
    seen, uniq = set(), []
    for b in out:
        assert 0 <= b[0] <= b[2] <= h and 0 <= b[1] <= b[3] <= w, (b, h, w)
        if b not in seen:
            seen.add(b)
            uniq.append(b)
    return uniq


def _pool(h, w):
    """(mode, box, fill) an image cycles through: every box as CONST and as NOISE, and NONE"""
    pool = [NO_BOX]
    for i, b in enumerate(_boxes(h, w)):
        pool.append((R.CONST, b, ((37 * i + 1) % 256, (91 * i + 2) % 256, (173 * i + 255) % 256)))
        pool.append((R.NOISE, b, (0, 0, 0)))
    return pool


def _batch(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)


SHAPES = [(1, 1, 1), (2, 5, 7), (3, 17, 37), (4, 32, 48), (2, 224, 224)]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_erase_kernel_bytes(n, h, w, off):
    """every box of _boxes as CONST and as NOISE, and NONE, each on a fresh batch: the whole canary buffer equals the restatement's.
    off = 1: the same from a base pointer one byte off the 16-byte grid"""
    x = _batch(n, h, w, n * 1000 + h)
    pool = _pool(h, w)
    if w > 16:
        assert any(m == R.NOISE and b[1] % 8 and b[3] % 8 and b[3] - b[1] > 16 for m, b, _ in pool)
    rounds = -(-len(pool) // n)
    seen = set()
    for r in range(rounds):
        items = [pool[(r * n + k) % len(pool)] for k in range(n)]
        seen |= {it[0] for it in items}
        got = _run(x, [(items, 0)], off)
        for k, (mode, (y0, x0, y1, x1), _) in enumerate(items):
            if mode == R.NOISE and (y1 - y0) * (x1 - x0) >= 64:
                assert not np.array_equal(got[k, 0, y0:y1, x0:x1], got[k, 1, y0:y1, x0:x1])           # planes draw independently
    assert seen == {R.NONE, R.CONST, R.NOISE}


def test_erase_two_positions_later_wins_and_positions_differ():
    n, h, w = 3, 17, 37
    x = _batch(n, h, w, 21)
    first = [(R.CONST, (2, 3, 12, 30), (10, 20, 30)), (R.NOISE, (0, 0, h, w), (0, 0, 0)), (R.CONST, (0, 0, h, w), (1, 1, 1))]
    second = [(R.NOISE, (6, 10, 17, 37), (0, 0, 0)), (R.CONST, (4, 5, 9, 22), (200, 100, 50)), NO_BOX]
    got = _run(x, [(first, 0), (second, 1)])
    assert bool((got[0, 0, 2:6, 3:30] == 10).all()) and bool((got[1, 2, 4:9, 5:22] == 50).all()) and bool((got[2] == 1).all())
    assert not bool((got[0, 0, 6:12, 10:30] == 10).all())                       # the overlap belongs to the later box
    # the same NOISE box at k = 0 and at k = 1: different bytes, each the restatement's
    box = [(R.NOISE, (1, 2, 15, 33), (0, 0, 0))] * n
    k0, k1 = _run(x, [(box, 0)]), _run(x, [(box, 1)])
    assert not np.array_equal(k0[:, :, 1:15, 2:33], k1[:, :, 1:15, 2:33])
    # position 1 then position 0 on the same box: the last launch's bytes
    assert np.array_equal(_run(x, [(box, 1), (box, 0)]), k0)


def test_erase_seeds():
    n, h, w = 2, 32, 48
    x = _batch(n, h, w, 22)
    box = [(R.NOISE, (3, 5, 30, 47), (0, 0, 0))] * n
    a, a2 = _run(x, [(box, 0)], seed=1), _run(x, [(box, 0)], seed=1)
    assert np.array_equal(a, a2)
    for other in (2, 1 + (1 << 32), (1 << 64) - 1):                             # low word, high word, all ones
        b = _run(x, [(box, 0)], seed=other)
        assert not np.array_equal(a[:, :, 3:30, 5:47], b[:, :, 3:30, 5:47])


def test_erase_refused_items_write_nothing():
    """a NOISE item with a null table, and descriptors the kernel must refuse: not one byte of their images changes, and the other
    images of the batch are still processed"""
    lib = L.load()
    host_tab, dev_tab = _table()
    n, h, w = 4, 32, 48
    x = _batch(n, h, w, 23)
    good = [(R.CONST, (3, 5, 20, 41), (9, 8, 7)), (R.NOISE, (0, 0, h, w), (0, 0, 0)), (R.NOISE, (7, 1, 30, 18), (0, 0, 0)),
            (R.CONST, (0, 0, h, 7), (255, 0, 128))]
    # null table: every NOISE item is refused, the CONST items run (the restatement sees the refused ones as NONE)
    size = x.size
    buf = torch.full((size + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
    buf[PAD:PAD + size].copy_(torch.from_numpy(x.reshape(-1)))
    _launch(buf, 0, x.shape, _arr(good), SEED, 0, None)
    want = R.erase_position(x.copy(), [it if it[0] == R.CONST else NO_BOX for it in good], host_tab, SEED, 0)
    got = buf.cpu().numpy()
    assert bool((got[:PAD] == CANARY).all()) and bool((got[PAD + size:] == CANARY).all())
    assert np.array_equal(got[PAD:PAD + size].reshape(x.shape), want)
    assert np.array_equal(want[1], x[1]) and np.array_equal(want[2], x[2]) and not np.array_equal(want[0], x[0])
    # one bad field at a time
    full = R.erase_position(x.copy(), good, host_tab, SEED, 0)
    for bad_at, field, val in [(0, "mode", 3), (1, "mode", -1), (1, "y1", h + 1), (1, "x1", w + 1), (2, "y0", 31), (2, "x0", 19),
                               (3, "y0", -1), (3, "x0", -1), (0, "pad", 1), (2, "pad", 255), (1, "reserved", (1, 0)),
                               (3, "reserved", (0, -1))]:
        arr = _arr(good)
        if field == "reserved":
            arr[bad_at].reserved[0], arr[bad_at].reserved[1] = val
        else:
            setattr(arr[bad_at], field, val)
        assert lib.mnas_img_erase_check(arr, n, h, w) == L.EINVAL, (field, val)
        buf = torch.full((size + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
        buf[PAD:PAD + size].copy_(torch.from_numpy(x.reshape(-1)))
        _launch(buf, 0, x.shape, arr, SEED, 0, dev_tab)
        got = buf.cpu().numpy()
        assert bool((got[:PAD] == CANARY).all()) and bool((got[PAD + size:] == CANARY).all()), (field, val)
        got = got[PAD:PAD + size].reshape(x.shape)
        for k in range(n):
            assert np.array_equal(got[k], x[k] if k == bad_at else full[k]), (field, val, k)


@pytest.mark.parametrize("kw", [dict(prob=0.6, mode="pixel"), dict(prob=0.7, mode="rand", min_count=1, max_count=3),
                                dict(prob=1.0, mode="const", value=(12, 34, 56), min_count=2),
                                dict(prob=1.0, mode="pixel", min_count=2, max_count=3, mean=(0.4, 0.5, 0.6), std=(0.1, 0.3, 0.2))])
def test_device_random_erasing_matches_restatement(kw):
    from mnasnet_pytorch_amd import DeviceRandomErasing
    n, h, w = 6, 40, 56
    x = _batch(n, h, w, 24)
    er = DeviceRandomErasing(**kw)
    tab = R.table(kw.get("mean", R.IMAGENET_MEAN), kw.get("std", R.IMAGENET_STD))
    for seed in (0, 1):
        random.seed(seed)
        draws, noise_seed = R.describe(n, h, w, **kw)
        after = random.random()
        assert any(draws)
        random.seed(seed)
        xd = torch.from_numpy(x).cuda()
        out = er(xd)
        assert random.random() == after
        assert out is xd                                                         # in place: the tensor it was given
        assert np.array_equal(out.cpu().numpy(), R.erase_batch(x, draws, tab, noise_seed))
    # explicit draws; no box at all and an empty batch are nothing to do
    xd = torch.from_numpy(x).cuda()
    assert er.apply(xd, [[]] * n, 5) is xd and np.array_equal(xd.cpu().numpy(), x)
    empty = torch.empty((0, 3, h, w), dtype=torch.uint8, device="cuda")
    assert er(empty) is empty
    from mnasnet_pytorch_amd.erasing import EraseBox
    with pytest.raises(ValueError):
        er.apply(xd, [[EraseBox(R.CONST, (0, 0, h + 1, w), (0, 0, 0))]] + [[]] * (n - 1), 5)          # the host check
    with pytest.raises(ValueError):
        er.apply(xd.float(), [[]] * n, 5)
    with pytest.raises(ValueError):
        er.apply(xd[:, :, :, ::2], [[]] * n, 5)
    with pytest.raises(ValueError):
        er.apply(xd, [[]] * (n - 1), 5)
    with pytest.raises(RuntimeError):
        er(xd.cpu())
    assert np.array_equal(xd.cpu().numpy(), x)                                   # nothing was launched by a refused call


def test_step_on_device_erased_batch_bit_equal_to_host_erased():
    """one Trainer.step on a uint8 batch erased by DeviceRandomErasing.apply from explicit draws against the same step on the
    batch the restatement erased on the host: same bytes, bit-equal loss and parameters.  The labels are untouched, so the trainer
    takes the batch as any other."""
    from mnasnet_pytorch_amd import DeviceRandomErasing
    from mnasnet_pytorch_amd.erasing import EraseBox
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_mix import _model
    x = _batch(4, 64, 64, 25)
    t = torch.tensor([1, 3, 5, 7]).cuda()
    draws = [[EraseBox(R.NOISE, (5, 9, 40, 50), (0, 0, 0))], [], [EraseBox(R.CONST, (0, 20, 33, 64), (124, 116, 104)),
             EraseBox(R.NOISE, (20, 3, 60, 31), (0, 0, 0))], [EraseBox(R.NOISE, (1, 1, 63, 63), (0, 0, 0))]]
    er = DeviceRandomErasing()
    res = []
    for route in ("device", "host"):
        if route == "device":
            xe = er.apply(torch.from_numpy(x).cuda(), draws, SEED)
        else:
            xe = torch.from_numpy(R.erase_batch(x, [[tuple(b) for b in boxes] for boxes in draws], R.table(), SEED)).cuda()
        tr = Trainer(_model(u8=True), lr=1e-3)
        assert tr._native_head() is not None
        loss = tr.step(xe, t)
        torch.cuda.synchronize()
        res.append((xe.cpu(), loss.clone(), tr.flat_p.clone()))
    assert torch.equal(res[0][0], res[1][0]) and not np.array_equal(res[0][0].numpy(), x)
    assert torch.equal(res[0][1], res[1][1]) and bool(torch.isfinite(res[0][1]))
    assert torch.equal(res[0][2], res[1][2])
