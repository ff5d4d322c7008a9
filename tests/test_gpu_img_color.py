"""-m gpu: the photometric image ops (csrc/mnas_imgc.hip) and preprocessing type 3 (DevicePipeline) on the MI355X.  Bytes equal
the Pillow golden (tests/golden/img_color.npz) and the numpy restatement (tests/img_color_ref.py, held to Pillow by the CPU
tests): every op over all 2^24 RGB triples, all 24 jitter orders, every layout pair, in place, odd sizes (the byte path), a
type-3 batch of mixed sources.  Every output lies inside a larger buffer whose bytes around it must not change, and out-of-place
calls run twice over two fill bytes and must agree (every byte written).  End to end, one Trainer step on a device-built type-3
batch is bit-equal to one on the host-built batch."""
import contextlib
import ctypes
import io
import itertools
import os
import random

import numpy as np
import pytest
import torch

import cases as C
import img_color_ref as R
from cases import O

pytestmark = pytest.mark.gpu

G = os.path.join(C.GOLDEN_DIR, "img_color.npz")
PAD = 4096                                     # canary bytes on each side of an output


def _lib():
    from mnasnet_pytorch_amd import _lib as L
    return L, L.load()


def _items(rows):
    """MnasImgColor array from (ops, factors, hue_shift) rows"""
    L, _ = _lib()
    arr = (L.MnasImgColor * max(1, len(rows)))()
    for k, (ops, fac, shift) in enumerate(rows):
        arr[k].nops = len(ops)
        for j, op in enumerate(ops):
            arr[k].op[j] = int(op)
            arr[k].factor[j] = float(fac[j]) if j < len(fac) else 0.0
        arr[k].hue_shift = int(shift)
    return arr


def _shape(layout, n, h, w):
    return (n, 3, h, w) if layout == 0 else (n, h, w, 3)


def _to_layout(imgs_hwc, layout):
    a = np.stack(imgs_hwc)
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2) if layout == 0 else a)


def _from_layout(a, layout):
    return a.transpose(0, 2, 3, 1) if layout == 0 else a


def _guarded_run(x, rows, il, ol):
    """out-of-place color_apply into the middle of a canary buffer, twice over two fill bytes -> output (host, layout ol)"""
    from mnasnet_pytorch_amd.transforms import color_apply
    n = x.shape[0]
    h, w = (x.shape[2], x.shape[3]) if il == 0 else (x.shape[1], x.shape[2])
    size = n * 3 * h * w
    outs = []
    for fill in (0x5A, 0xA5):
        buf = torch.full((size + 2 * PAD,), fill, dtype=torch.uint8, device="cuda")
        out = buf[PAD:PAD + size].view(_shape(ol, n, h, w))
        color_apply(x, _items(rows), il, ol, out=out)
        b = buf.cpu()
        assert bool((b[:PAD] == fill).all()) and bool((b[PAD + size:] == fill).all()), "write outside the output"
        outs.append(b[PAD:PAD + size].view(_shape(ol, n, h, w)).numpy().copy())
    assert np.array_equal(outs[0], outs[1]), "bytes left unwritten"
    return outs[0]


def test_kernel_matches_pillow_golden():
    g = np.load(G)
    src = g["op_src"]
    rows = []
    for r in g["op_cases"]:
        nops = int(r[0])
        rows.append(([int(v) for v in r[1:1 + nops]], [float(v) for v in r[6:6 + nops]], int(r[11])))
    for il, ol in [(0, 1), (1, 0)]:
        x = torch.from_numpy(_to_layout([src] * len(rows), il)).cuda()
        got = _from_layout(_guarded_run(x, rows, il, ol), ol)
        for k in range(len(rows)):
            assert np.array_equal(got[k], g["op_out"][k]), (k, rows[k])
    # the type-3 batch: same seed, same draws, Pillow's bytes
    from mnasnet_pytorch_amd import DevicePipeline, ImageBatch
    meta = g["t3_meta"]
    batch = ImageBatch(torch.from_numpy(g["t3_src"].copy()), [tuple(m[1:]) for m in meta], [int(m[0]) for m in meta]).to("cuda")
    random.seed(int(g["t3_seed"]))
    out = DevicePipeline.from_reference(3, final_size=tuple(g["t3_size"]), prob=float(g["t3_prob"]))(batch).cpu().numpy()
    assert np.array_equal(out, g["t3_out"])


@pytest.fixture(scope="module")
def cube():
    return R.cube_image(), R.CubeTables()


def test_every_op_over_the_rgb_cube(cube):
    img, tab = cube
    x = torch.from_numpy(img[None]).cuda()                         # one 4096 x 4096 NHWC image: every RGB triple once
    runs = [([R.BRIGHTNESS], [0.93]), ([R.BRIGHTNESS], [1.07]), ([R.CONTRAST], [0.93]), ([R.CONTRAST], [1.07]),
            ([R.SATURATION], [0.93]), ([R.SATURATION], [1.07]), ([R.GRAY], [0.0])]
    for ops, fac in runs:
        got = _guarded_run(x, [(ops, fac, 0)], 1, 1)[0]
        assert np.array_equal(got, R.color(img, ops, fac)), (ops, fac)
    for shift in (3, 128, 231, 255):
        got = _guarded_run(x, [([R.HUE], [0.0], shift)], 1, 1)[0]
        assert np.array_equal(got, tab.hue(img, shift)), shift


def test_all_24_orders_and_layouts():
    rng = np.random.default_rng(5)
    perms = list(itertools.permutations([R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE]))
    for h, w in [(64, 96), (61, 83)]:                               # H*W % 16 == 0 (16-byte path) and not (byte path)
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in perms]
        rows = []
        for p in perms:
            fac = [float(v) for v in rng.uniform(0.88, 1.12, 4)]
            rows.append((list(p), fac, int(rng.integers(0, 256))))
        want = [R.color(a, *r) for a, r in zip(imgs, rows)]
        for il, ol in itertools.product((0, 1), (0, 1)):
            x = torch.from_numpy(_to_layout(imgs, il)).cuda()
            got = _from_layout(_guarded_run(x, rows, il, ol), ol)
            for k in range(len(perms)):
                assert np.array_equal(got[k], want[k]), (h, w, il, ol, rows[k])


def test_in_place_leaves_nops0_items_alone():
    from mnasnet_pytorch_amd.transforms import color_apply
    rng = np.random.default_rng(6)
    for h, w in [(48, 64), (37, 29)]:
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(6)]
        rows = [([], [], 0), ([R.GRAY], [0.0], 0), ([], [], 0), ([R.CONTRAST, R.HUE], [1.3, 0.0], 200), ([], [], 0),
                ([R.SATURATION], [0.0], 0)]
        want = [R.color(a, *r) for a, r in zip(imgs, rows)]
        for layout in (0, 1):
            size = 6 * 3 * h * w
            buf = torch.full((size + 2 * PAD,), 0x77, dtype=torch.uint8, device="cuda")
            x = buf[PAD:PAD + size].view(_shape(layout, 6, h, w))
            x.copy_(torch.from_numpy(_to_layout(imgs, layout)))
            color_apply(x, _items(rows), layout, layout, out=x)
            b = buf.cpu()
            assert bool((b[:PAD] == 0x77).all()) and bool((b[PAD + size:] == 0x77).all())
            got = _from_layout(b[PAD:PAD + size].view(_shape(layout, 6, h, w)).numpy(), layout)
            for k in range(6):
                assert np.array_equal(got[k], want[k]), (h, w, layout, k)


def test_refused_item_writes_nothing():
    """a descriptor the host check would refuse, sent straight to the device: its image is not written, its neighbours are"""
    L, lib = _lib()
    rng = np.random.default_rng(7)
    h, w = 32, 48
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(4)]
    rows = [([R.BRIGHTNESS], [1.2], 0), ([R.HUE], [0.0], 9), ([R.CONTRAST], [0.8], 0), ([R.SATURATION], [0.5], 0)]
    for bad_at, field, ws_too in [(1, "op", True), (2, "reserved", True), (3, "hue_shift", True), (2, None, False)]:
        arr = _items(rows)
        if field == "op":
            arr[bad_at].op[0] = 9
        elif field == "reserved":
            arr[bad_at].reserved = 1
        elif field == "hue_shift":
            arr[bad_at].hue_shift = 256
        x = torch.from_numpy(_to_layout(imgs, 0)).cuda()
        out = torch.full((4, 3, h, w), 0x3C, dtype=torch.uint8, device="cuda")
        items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
        ws = torch.empty(lib.mnas_img_color_workspace_bytes(4, h, w), dtype=torch.uint8, device="cuda") if ws_too else None
        L.check(lib.mnas_img_color(items.data_ptr(), 4, h, w, 0, x.data_ptr(), 0, out.data_ptr(), L.ptr(ws), L.cur_stream()))
        got = out.cpu().numpy().transpose(0, 2, 3, 1)
        for k in range(4):
            if k == bad_at:
                assert bool((got[k] == 0x3C).all()), (field, k)      # without a workspace a CONTRAST item is refused too
            else:
                assert np.array_equal(got[k], R.color(imgs[k], *rows[k])), (field, k)


def test_same_size_xform_is_identity():
    """what the type-3 chain relies on for images not jittered: a whole-image same-size bilinear resample copies the image"""
    from mnasnet_pytorch_amd import ImageBatch
    from mnasnet_pytorch_amd.transforms import apply
    rng = np.random.default_rng(8)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(224, 224), (384, 512), (37, 61), (1, 5)]]
    for img in imgs:
        h, w = img.shape[:2]
        b = ImageBatch.from_arrays([img]).to("cuda")
        out = apply(b, [(0, 0, h, w, h, w, 0, 0, 0)], (h, w)).cpu().numpy()[0]
        assert np.array_equal(out, img.transpose(2, 0, 1)), (h, w)


def _sources(rng, n, lo, hi):
    imgs = []
    for k in range(n):
        h, w = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        c = int(rng.choice([1, 3, 4]))
        imgs.append(rng.integers(0, 256, (h, w) if c == 1 and k % 2 else (h, w, c), dtype=np.uint8))
    return imgs


def test_type3_pipeline_matches_restatement():
    from mnasnet_pytorch_amd import DevicePipeline, ImageBatch
    from mnasnet_pytorch_amd.transforms import run_type3
    rng = np.random.default_rng(9)
    seen = set()
    for prob, size, seed in [(1.0, (96, 128), 1), (0.5, (61, 47), 2), (0.2, (128, 96), 3)]:
        imgs = _sources(rng, 24, 40, 260)
        batch = ImageBatch.from_arrays(imgs)
        random.seed(seed)
        hw, draws = DevicePipeline.from_reference(3, final_size=size, prob=prob).describe(batch.shapes)
        out = run_type3(batch.to("cuda", non_blocking=True), draws, hw).cpu().numpy()
        assert out.shape == (24, 3) + size
        for k, (img, d) in enumerate(zip(imgs, draws)):
            assert np.array_equal(out[k], R.type3(img, size, d)), (prob, k, img.shape, d)
            seen.add((d.applied, d.flags, d.gray))
    assert {a for a, _, _ in seen} == {False, True} and {g for _, _, g in seen} == {False, True}
    assert {f for _, f, _ in seen} == {0, 1, 2, 3}


def _build(cfg="512", num_classes=10):
    from mnasnet_pytorch_amd import FineTuneModelPool, load_model
    with contextlib.redirect_stdout(io.StringIO()):
        base = load_model("mnasnet")
    m = FineTuneModelPool(base, "mnasnet", num_classes, cfg)
    m.load_state_dict({**O.init_state(False, C.STATE_SEED, proj_gamma=0.1), **O.init_head_state(cfg, num_classes, C.STATE_SEED)})
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m.cuda()


def test_trainer_step_bit_equal_to_host_pipeline():
    """one Trainer.step on a small 384 x 512 cluster batch of preprocessing type 3 (prob 1.0: every image jittered, cropped,
    flipped and greyed) leaves bit-equal parameters whether the batch was built on the device or by the restatement on the
    host and uploaded."""
    from mnasnet_pytorch_amd import DevicePipeline, ImageBatch
    from mnasnet_pytorch_amd.train_step import Trainer
    rng = np.random.default_rng(10)
    imgs = _sources(rng, 4, 300, 700)
    pipe = DevicePipeline.from_reference(3, prob=1.0)
    target = torch.tensor([1, 3, 5, 7]).cuda()
    params = []
    for route in ("device", "host"):
        random.seed(99)
        batch = ImageBatch.from_arrays(imgs, target_size=(384, 512))
        if route == "device":
            x = pipe(batch.to("cuda", non_blocking=True))
        else:
            hw, draws = pipe.describe(batch.shapes, batch.target_size)
            x = torch.from_numpy(np.stack([R.type3(a, hw, d) for a, d in zip(imgs, draws)])).cuda()
        assert x.shape == (4, 3, 384, 512) and x.dtype == torch.uint8
        torch.manual_seed(0)
        m = _build().train()
        m.normalize_on_device()
        tr = Trainer(m, lr=1e-3)
        loss = tr.step(x, target)
        torch.cuda.synchronize()
        params.append((float(loss), [p.detach().clone() for p in m.parameters()]))
    assert params[0][0] == params[1][0]
    assert all(torch.equal(a, b) for a, b in zip(params[0][1], params[1][1]))


def test_host_check_agrees_with_the_launch_wrapper():
    """color_apply refuses what mnas_img_color_check refuses, before any launch"""
    from mnasnet_pytorch_amd.transforms import color_apply
    x = torch.zeros((2, 3, 8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        color_apply(x, _items([([R.CONTRAST, R.CONTRAST], [1.0, 1.0], 0), ([], [], 0)]), 0, 0)
    with pytest.raises(ValueError):
        color_apply(x, [[], []], 0, 1, out=x)                      # in place across layouts
    assert ctypes.sizeof(_lib()[0].MnasImgColor) == 52
