"""-m gpu: the augmentation-policy ops (csrc/mnas_imga.hip) and DeviceRandAugment on the MI355X.  Bytes equal the Pillow golden
(tests/golden/randaug.npz) and the numpy restatement (tests/randaug_ref.py, held to Pillow by the CPU tests): every op alone and
in chains of 0 to 4 ops, with and without statistics ops and with two of them in one chain, on shapes that take the 16-byte path
(64 x 96; 32 x 24, whose rows are no multiple of 16 bytes), the byte path (61 x 83), the filter's border and its < 3 case (3 x 3,
2 x 7) and two statistics chunks (160 x 128).
Every output lies inside a larger buffer whose bytes around it must not change, and every run is made twice over two fill bytes
and must agree (every byte written).  A refused descriptor leaves its image unwritten.  End to end, one Trainer step on a
device-augmented batch is bit-equal to one on the batch the restatement built on the host."""
import contextlib
import ctypes
import io
import os
import random

import numpy as np
import pytest
import torch

import cases as C
import randaug_ref as A
from cases import O

pytestmark = pytest.mark.gpu

G = os.path.join(C.GOLDEN_DIR, "randaug.npz")
PAD = 4096                                     # canary bytes on each side of an output
SHAPES = [(64, 96), (61, 83), (3, 3), (2, 7), (160, 128), (32, 24)]


def _lib():
    from mnasnet_pytorch_amd import _lib as L
    return L, L.load()


def _nchw(imgs_hwc):
    return np.ascontiguousarray(np.stack(imgs_hwc).transpose(0, 3, 1, 2))


def _guarded_run(x, items, fill=(0, 0, 0)):
    """aug_apply into the middle of a canary buffer, twice over two fill bytes -> output (host, NHWC)"""
    from mnasnet_pytorch_amd import aug_apply
    size = x.numel()
    outs = []
    for canary in (0x5A, 0xA5):
        buf = torch.full((size + 2 * PAD,), canary, dtype=torch.uint8, device="cuda")
        out = buf[PAD:PAD + size].view(x.shape)
        aug_apply(x, items, fill, out=out)
        b = buf.cpu()
        assert bool((b[:PAD] == canary).all()) and bool((b[PAD + size:] == canary).all()), "write outside the output"
        outs.append(b[PAD:PAD + size].view(x.shape).numpy().copy())
    assert np.array_equal(outs[0], outs[1]), "bytes left unwritten"
    return outs[0].transpose(0, 2, 3, 1)


def _ops(rows):
    """golden rows (source, code, factor, six arguments) -> [(source, (code, factor, args))]"""
    return [(int(r[0]), (int(r[1]), float(r[2]), tuple(int(v) for v in r[3:9]))) for r in rows]


def test_kernel_matches_pillow_golden():
    g = np.load(G)
    src, fill = g["src"], tuple(int(v) for v in g["fill"])
    singles = _ops(g["op_cases"])
    x = torch.from_numpy(_nchw([src[s] for s, _ in singles])).cuda()
    got = _guarded_run(x, [[op] for _, op in singles], fill)
    for k, (_, op) in enumerate(singles):
        assert np.array_equal(got[k], g["op_out"][k]), (k, op)
    # the two-op chains and the seeded batch's descriptors in one launch
    rows = [_ops(r) for r in list(g["chain_cases"]) + list(g["ra_cases"])]
    want = list(g["chain_out"]) + list(g["ra_out"])
    x = torch.from_numpy(_nchw([src[r[0][0]] for r in rows])).cuda()
    got = _guarded_run(x, [[op for _, op in r] for r in rows], fill)
    for k in range(len(rows)):
        assert np.array_equal(got[k], want[k]), (k, rows[k])
    # the same seed through DeviceRandAugment: same draws, Pillow's bytes
    from mnasnet_pytorch_amd import DeviceRandAugment
    x = torch.from_numpy(_nchw([src[int(s)] for s in g["ra_src"]])).cuda()
    random.seed(int(g["ra_seed"]))
    out = DeviceRandAugment(2, 9, fill=fill)(x).cpu().numpy().transpose(0, 2, 3, 1)
    assert np.array_equal(out, g["ra_out"])


def _single_ops(h, w):
    """every op alone, the affine ones as shear, rotation, translation and a warp that leaves the image entirely"""
    ops = [(A.AFFINE, 0.0, A.fixed_matrix(m)) for m in [(1, 0.3, 0, 0, 1, 0), (1, 0, 0, -0.27, 1, 0), A.rotate_matrix(23.5, h, w),
                                                       A.rotate_matrix(-141.0, h, w), (1, 0, max(1, w // 3), 0, 1, 0),
                                                       (1, 0, 0, 0, 1, -max(1, h // 4)), (1, 0, 3 * w, 0, 1, 0)]]
    ops += [(code, f, ()) for code in (A.BRIGHTNESS, A.COLOR, A.CONTRAST, A.SHARPNESS) for f in (0.1, 1.9)]
    ops += [(A.SHARPNESS, 1.0, ()), (A.POSTERIZE, 0.0, (4,)), (A.POSTERIZE, 0.0, (8,)), (A.POSTERIZE, 0.0, (1,)), (A.SOLARIZE, 0.0, (0,)),
            (A.SOLARIZE, 0.0, (128,)), (A.SOLARIZE, 0.0, (255,)), (A.INVERT, 0.0, ()), (A.AUTOCONTRAST, 0.0, ()), (A.EQUALIZE, 0.0, ()),
            (A.IDENTITY, 0.0, ())]
    return ops


def _mixed_chains(h, w):
    """chain lengths 0..4 in one batch, with and without statistics ops, two statistics ops in one chain, statistics ops at
    every position of a chain (chains are right-aligned, so at every stage)"""
    shear, rot = (A.AFFINE, 0.0, A.fixed_matrix((1, -0.21, 0, 0, 1, 0))), (A.AFFINE, 0.0, A.fixed_matrix(A.rotate_matrix(-17.0, h, w)))
    eq, ac, inv, sol = (A.EQUALIZE, 0.0, ()), (A.AUTOCONTRAST, 0.0, ()), (A.INVERT, 0.0, ()), (A.SOLARIZE, 0.0, (100,))
    con, sharp, col, post = (A.CONTRAST, 1.6, ()), (A.SHARPNESS, 1.9, ()), (A.COLOR, 0.3, ()), (A.POSTERIZE, 0.0, (3,))
    return [[], [eq, ac], [inv], [shear, sharp, con, eq], [sol, post], [], [ac, rot, eq], [con], [sharp, sharp, sharp, sharp],
            [eq, ac, con, ac], [rot, shear], [col, con, inv], [ac], [(A.IDENTITY, 0.0, ())], [eq, eq], [post, inv, sol, col]]


def _images(rng, n, h, w):
    """random images; every third one low-contrast, every fifth with a constant and a two-valued channel"""
    imgs = []
    for k in range(n):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 3 == 1:
            a = (a // 4 + 90).astype(np.uint8)
        if k % 5 == 2:
            a[..., 0] = 201
            a[..., 2] = np.where(rng.random((h, w)) < 0.4, 30, 220)
        imgs.append(a)
    return imgs


@pytest.mark.parametrize("h,w", SHAPES)
def test_every_op_and_mixed_chains_against_restatement(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    fill = (11, 250, 128)
    for rows in ([[op] for op in _single_ops(h, w)], _mixed_chains(h, w)):
        imgs = _images(rng, len(rows), h, w)
        got = _guarded_run(torch.from_numpy(_nchw(imgs)).cuda(), rows, fill)
        for k, (img, ops) in enumerate(zip(imgs, rows)):
            assert np.array_equal(got[k], A.chain(img, ops, fill)), (h, w, k, ops)


def test_refused_item_writes_nothing():
    """a descriptor the host check would refuse, sent straight to the device: its image is not written, its neighbours are"""
    from mnasnet_pytorch_amd import aug_apply
    from mnasnet_pytorch_amd import augment as AU
    L, lib = _lib()
    rng = np.random.default_rng(7)
    h, w = 32, 48
    imgs = _images(rng, 5, h, w)
    shear = A.fixed_matrix((1, 0.3, 0, 0, 1, 0))
    rows = [[(A.BRIGHTNESS, 1.2, ()), (A.EQUALIZE, 0.0, ())], [(A.POSTERIZE, 0.0, (5,)), (A.INVERT, 0.0, ())],
            [(A.AFFINE, 0.0, shear), (A.CONTRAST, 0.8, ())], [(A.SHARPNESS, 0.5, ())], []]
    x = torch.from_numpy(_nchw(imgs)).cuda()
    for bad_at, field in [(1, "op"), (3, "reserved"), (1, "bits"), (2, "matrix"), (2, "translation")]:
        arr = AU.aug_items(rows)
        if field == "op":
            arr[bad_at].op[0] = 11
        elif field == "reserved":
            arr[bad_at].reserved = 1
        elif field == "bits":
            arr[bad_at].arg[0][0] = 9
        elif field == "matrix":
            arr[bad_at].arg[0][0] = 1 << 30                       # x a0 leaves the int32 fixed-point range inside the image
        else:
            arr[bad_at].arg[0][1] = 0                             # a1 == a3 == 0 but no whole-pixel translation (a2 = 32768 + 0.15 * 65536)
            arr[bad_at].arg[0][2] = 32768 + 9830
        assert lib.mnas_img_aug_check(arr, 5, h, w) == L.EINVAL, field
        with pytest.raises(ValueError):
            aug_apply(x, arr)                                      # the wrapper refuses before launching
        max_ops, stages = AU.aug_plan(arr, 5)
        assert (max_ops, stages) == (2, 0b10)
        out = torch.full((5, 3, h, w), 0x3C, dtype=torch.uint8, device="cuda")
        items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
        ws = torch.empty(lib.mnas_img_aug_workspace_bytes(5, h, w, max_ops, 1), dtype=torch.uint8, device="cuda")
        L.check(lib.mnas_img_aug(items.data_ptr(), 5, h, w, max_ops, stages, 0, x.data_ptr(), out.data_ptr(), L.ptr(ws), L.cur_stream()))
        got = out.cpu().numpy().transpose(0, 2, 3, 1)
        for k in range(5):
            if k == bad_at:
                assert bool((got[k] == 0x3C).all()), (field, k)
            else:
                assert np.array_equal(got[k], A.chain(imgs[k], rows[k])), (field, k)
    # a plan that does not cover the descriptors refuses them too: a chain longer than max_ops, a statistics op without its launch
    arr = AU.aug_items(rows)
    out = torch.full((5, 3, h, w), 0x3C, dtype=torch.uint8, device="cuda")
    items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
    ws = torch.empty(lib.mnas_img_aug_workspace_bytes(5, h, w, 2, 1), dtype=torch.uint8, device="cuda")
    L.check(lib.mnas_img_aug(items.data_ptr(), 5, h, w, 1, 0, 0, x.data_ptr(), out.data_ptr(), L.ptr(ws), L.cur_stream()))
    got = out.cpu().numpy().transpose(0, 2, 3, 1)
    for k in range(5):
        if len(rows[k]) > 1:
            assert bool((got[k] == 0x3C).all()), k
        else:
            assert np.array_equal(got[k], A.chain(imgs[k], rows[k])), k


def test_launch_wrapper_refuses_before_launching():
    from mnasnet_pytorch_amd import DeviceRandAugment, aug_apply
    L, _ = _lib()
    assert ctypes.sizeof(L.MnasImgAug) == 136
    x = torch.zeros((2, 3, 8, 8), dtype=torch.uint8, device="cuda")
    for bad in ([(11, 0.0, ())], [(A.POSTERIZE, 0.0, (0,))], [(A.BRIGHTNESS, -1.0, ())], [(A.AFFINE, 0.0, (1 << 30, 1, 0, 0, 65536, 0))],
                [(A.AFFINE, 0.0, (98304, 0, 32768, 0, 65536, 32768))]):
        with pytest.raises(ValueError):
            aug_apply(x, [[], bad])
    with pytest.raises(ValueError):
        aug_apply(x, [[]])                                         # one descriptor per image
    with pytest.raises(ValueError):
        aug_apply(x, [[], []], out=x)                              # out of place only
    with pytest.raises(ValueError):
        aug_apply(x, [[], []], fill=(0, 0, 300))
    with pytest.raises(ValueError):
        aug_apply(x.float(), [[], []])
    with pytest.raises(RuntimeError):
        DeviceRandAugment()(x.cpu())
    empty = aug_apply(x[:0], [])
    assert empty.shape == (0, 3, 8, 8)
    assert torch.equal(aug_apply(x + 7, [[], [(A.INVERT, 0.0, ())]]), torch.stack([x[0] + 7, 248 - x[1]]))


def test_seeded_randaugment_matches_restatement():
    from mnasnet_pytorch_amd import DeviceRandAugment
    rng = np.random.default_rng(9)
    h, w, fill = 61, 83, (128, 128, 128)
    imgs = _images(rng, 24, h, w)
    ra = DeviceRandAugment(2, 9, fill=fill)
    random.seed(8)                                                 # chosen on the CPU: these 48 draws meet every op under every sign
    rows = ra.describe(24, (h, w))
    seen = {(o.name, o.sign) for r in rows for o in r}
    assert {n for n, _ in seen} == set(A.NAMES)
    assert seen == {(n, s) for n in A.NAMES for s in ((0, 1) if n in A.SIGNED else (0,))}
    x = torch.from_numpy(_nchw(imgs)).cuda()
    got = _guarded_run(x, rows, fill)
    for k, (img, r) in enumerate(zip(imgs, rows)):
        assert np.array_equal(got[k], A.chain(img, [(o.op, o.factor, o.args) for o in r], fill)), (k, r)
    random.seed(8)
    assert np.array_equal(ra(x).cpu().numpy().transpose(0, 2, 3, 1), got)          # the callable: the same draws, the same bytes


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


def test_trainer_step_bit_equal_to_host_augmentation():
    """one Trainer.step on a (4, 3, 96, 128) batch under DeviceRandAugment(2, 9) leaves bit-equal loss and parameters whether
    the batch was augmented on the device or by the restatement on the host and uploaded"""
    from mnasnet_pytorch_amd import DeviceRandAugment
    from mnasnet_pytorch_amd.train_step import Trainer
    rng = np.random.default_rng(10)
    imgs = _images(rng, 4, 96, 128)
    ra = DeviceRandAugment(2, 9)
    target = torch.tensor([1, 3, 5, 7]).cuda()
    params = []
    for route in ("device", "host"):
        random.seed(3)                                             # TranslateX, Rotate, Posterize, Sharpness x 2, Equalize, Color, Contrast
        if route == "device":
            x = ra(torch.from_numpy(_nchw(imgs)).cuda())
        else:
            rows = ra.describe(4, (96, 128))
            assert {o.name for r in rows for o in r} >= {"Rotate", "Sharpness", "Equalize", "Contrast"}
            x = torch.from_numpy(_nchw([A.chain(a, [(o.op, o.factor, o.args) for o in r]) for a, r in zip(imgs, rows)])).cuda()
        assert x.shape == (4, 3, 96, 128) and x.dtype == torch.uint8
        torch.manual_seed(0)
        m = _build().train()
        m.normalize_on_device()
        tr = Trainer(m, lr=1e-3)
        loss = tr.step(x, target)
        torch.cuda.synchronize()
        params.append((float(loss), [p.detach().clone() for p in m.parameters()]))
    assert params[0][0] == params[1][0]
    assert all(torch.equal(a, b) for a, b in zip(params[0][1], params[1][1]))
