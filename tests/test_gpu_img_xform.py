"""-m gpu: the image batch transform (csrc/mnas_imgx.hip) on the MI355X.  Its bytes equal the Pillow golden
(tests/golden/img_xform.npz) and the numpy restatement (tests/img_xform_ref.py, held to Pillow by the CPU tests) on mixed-size
batches up to 2000 px, every channel count, both flips, 224^2 / 384 x 512 / 512 x 384 / 97 x 61 outputs, a 30x downscale and a
256-image batch; end to end, a device-transformed batch and the same batch built on the host give torch.equal logits and one
bit-equal Trainer step.  Every descriptor launched here passes mnas_img_xform_check first (transforms.apply)."""
import contextlib
import io
import os
import random

import numpy as np
import pytest
import torch

import cases as C
import img_xform_ref as R
from cases import O

pytestmark = pytest.mark.gpu

G = os.path.join(C.GOLDEN_DIR, "img_xform.npz")


def _golden_batch(g):
    from mnasnet_pytorch_amd import ImageBatch
    meta = g["src_meta"]
    buf = torch.from_numpy(g["src"].copy())
    return ImageBatch(buf, [tuple(m[1:]) for m in meta], [int(m[0]) for m in meta]).to("cuda")


def _run_rows(gb, rows):
    """golden case rows (src, box, rsize, window, flags, Ho, Wo) of one output size -> kernel output (N, 3, Ho, Wo) on the host"""
    from mnasnet_pytorch_amd import ImageBatch
    from mnasnet_pytorch_amd.transforms import apply
    rows = [[int(v) for v in r] for r in rows]
    b = ImageBatch(gb.data, [gb.shapes[r[0]] for r in rows], [gb.offsets[r[0]] for r in rows])
    out = apply(b, [tuple(r[1:10]) for r in rows], (rows[0][10], rows[0][11]))
    return out.cpu()


def test_kernel_matches_pillow_golden():
    g = np.load(G)
    gb = _golden_batch(g)
    for k, row in enumerate(g["cases"]):
        got = _run_rows(gb, [row]).numpy().reshape(-1)
        o = int(g["out_off"][k])
        assert np.array_equal(got, g["out"][o:o + got.size]), (k, row.tolist())
    got = _run_rows(gb, g["e2e_cases"]).numpy()
    assert np.array_equal(got, g["e2e_out"])


def _sources(rng, n, lo, hi, big=0):
    imgs = []
    for k in range(n):
        if k < big:
            h, w = int(rng.integers(1500, 2001)), int(rng.integers(1500, 2001))
        else:
            h, w = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        c = int(rng.choice([1, 3, 4]))
        imgs.append(rng.integers(0, 256, (h, w) if c == 1 and k % 2 else (h, w, c), dtype=np.uint8))
    return imgs


def _check_against_restatement(imgs, tf, seed, size=None):
    from mnasnet_pytorch_amd import ImageBatch
    from mnasnet_pytorch_amd.transforms import apply
    batch = ImageBatch.from_arrays(imgs)
    random.seed(seed)
    hw, desc = tf.describe(batch.shapes, size)
    out = apply(batch.to("cuda", non_blocking=True), desc, hw).cpu().numpy()
    assert out.shape == (len(imgs), 3) + hw
    for k, (img, d) in enumerate(zip(imgs, desc)):
        want = R.xform(img, d[0:4], d[4:6], d[6:8], hw, d[8])
        assert np.array_equal(out[k], want), (k, img.shape, d)
    return desc


def test_kernel_matches_restatement_sweep():
    from mnasnet_pytorch_amd import DeviceTransform
    rng = np.random.default_rng(11)
    n = 0
    # RandomResizedCrop + both flips to 224^2, sources up to 2000 px
    d = _check_against_restatement(_sources(rng, 48, 16, 700, big=3),
                                   DeviceTransform("random_resized_crop", (224, 224), hflip=0.5, vflip=0.5), 1)
    assert {x[8] for x in d} == {0, 1, 2, 3}
    n += 48
    # whole-image resizes to the 384 x 512 / 512 x 384 clusters (up- and downscaling)
    for k, hw in enumerate([(384, 512), (512, 384)]):
        _check_against_restatement(_sources(rng, 14, 100, 900), DeviceTransform("resize", hw, hflip=0.5, vflip=0.5), 2 + k)
        n += 14
    # an odd output size, crops from 1 % of the area up
    _check_against_restatement(_sources(rng, 48, 8, 600),
                               DeviceTransform("random_resized_crop", (97, 61), scale=(0.01, 1.0), hflip=0.5, vflip=0.5), 4)
    n += 48
    # shorter side + centre crop (types 1), including windows at odd offsets
    _check_against_restatement(_sources(rng, 24, 40, 500), DeviceTransform.from_reference(1, fixed_size=(224, 224)), 5)
    n += 24
    # a 30x downscale: 1800 x 1950 -> 60 x 65
    imgs = [rng.integers(0, 256, (1800, 1950, c), dtype=np.uint8) for c in (3, 4, 1)]
    _check_against_restatement(imgs, DeviceTransform("resize", (60, 65), hflip=0.5), 6)
    n += 3
    # N = 256 at 224^2 in one call: the reference's type-5 geometry
    _check_against_restatement(_sources(rng, 256, 120, 520), DeviceTransform.from_reference(5), 7)
    n += 256
    assert n >= 200


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


def test_end_to_end_logits_equal_host_pipeline():
    """FineTuneModelPool logits on a device-transformed batch are torch.equal to logits on the same batch built by Pillow on
    the host (the golden's 8-image RandomResizedCrop + flip batch, 64 x 64) and uploaded as uint8."""
    g = np.load(G)
    gb = _golden_batch(g)
    x_dev = _run_rows(gb, g["e2e_cases"]).cuda()
    x_host = torch.from_numpy(g["e2e_out"]).cuda()
    assert torch.equal(x_dev, x_host) and x_dev.is_contiguous()
    m = _build().eval()
    m.normalize_on_device()
    with torch.no_grad():
        a = m(x_dev)
        b = m(x_host)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_trainer_step_bit_equal_to_host_pipeline():
    """one Trainer.step on a small 384 x 512 cluster batch (reference type 4: RandomResizedCropRect(final_size) + hflip) leaves
    bit-equal parameters whether the batch was transformed on the device or built on the host and uploaded."""
    from mnasnet_pytorch_amd import DeviceTransform, ImageBatch
    from mnasnet_pytorch_amd.train_step import Trainer
    rng = np.random.default_rng(5)
    imgs = _sources(rng, 4, 300, 700)
    tf = DeviceTransform.from_reference(4)
    target = torch.tensor([1, 3, 5, 7]).cuda()
    params = []
    for route in ("device", "host"):
        random.seed(99)
        batch = ImageBatch.from_arrays(imgs, target_size=(384, 512))
        if route == "device":
            x = tf(batch.to("cuda", non_blocking=True))
        else:
            hw, desc = tf.describe(batch.shapes, batch.target_size)
            x = torch.from_numpy(np.stack([R.xform(a, d[0:4], d[4:6], d[6:8], hw, d[8]) for a, d in zip(imgs, desc)])).cuda()
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
