"""CPU (no GPU needed): label smoothing and batch mixing.  The loss's closed form against F.cross_entropy in fp64; the integer
blend's properties over all byte pairs; the CutMix box and the weight it leaves; DeviceMix.describe under a seed against the
restatement of its documented draw order; mnas_img_mix_check (a host function) over accepted and refused descriptors; the Python
surface refuses CPU tensors and a MixedTarget handed to another criterion."""
import ctypes
import random
import types

import numpy as np
import pytest
import torch

import mix_ref as R


def test_closed_form_matches_f_cross_entropy():
    g = torch.Generator().manual_seed(3)
    for N, C in [(1, 1), (7, 10), (33, 257)]:
        z = torch.randn(N, C, generator=g, dtype=torch.float64) * 3
        a = torch.randint(0, C, (N,), generator=g)
        b = torch.randint(0, C, (N,), generator=g)
        lam = torch.rand(N, generator=g, dtype=torch.float64)
        lam[::4] = 1.0
        lam[1::4] = 0.0
        for eps in (0.0, 0.1):
            for mixed in (False, True):
                for ignore in (False, True):
                    aa, bb = a.clone(), b.clone()
                    if ignore and N > 2:
                        aa[0] = -100
                        bb[2] = -100
                    args = (z, aa, bb if mixed else None, lam if mixed else None, eps)
                    ref, gref = R.soft_ce(*args)
                    got, ggot = R.soft_ce_closed_form(*args)
                    assert abs(float(got) - float(ref)) < 1e-12, (N, C, eps, mixed, ignore)
                    assert float((ggot - gref).abs().max()) < 1e-14
    # every row ignored: NaN
    z = torch.randn(3, 4, dtype=torch.float64)
    t = torch.full((3,), -100)
    assert torch.isnan(R.soft_ce(z, t)[0]) and torch.isnan(R.soft_ce_closed_form(z, t)[0])


def test_integer_blend_properties():
    x, p = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(R.blend(x, p, 65536), x.astype(np.uint8))
    assert np.array_equal(R.blend(x, p, 0), p.astype(np.uint8))
    for w16 in (0, 1, 12345, 32768, 65535, 65536):
        wide = (w16 * x.astype(np.int64) + (65536 - w16) * p.astype(np.int64) + 32768) >> 16
        assert wide.min() >= 0 and wide.max() <= 255
        real = (w16 * x + (65536 - w16) * p) / 65536.0
        assert np.abs(wide - real).max() <= 0.5                 # correct rounding of the real-valued blend
        lo, hi = np.minimum(x, p), np.maximum(x, p)
        assert ((wide >= lo) & (wide <= hi)).all()


def test_box_formula_and_effective_weight():
    from mnasnet_pytorch_amd.mixing import cutmix_box
    assert cutmix_box(224, 224, 0.75, 112, 112) == ((56, 56, 168, 168), 0.75)       # r = 0.5: a centred 112 x 112 box
    assert cutmix_box(10, 20, 1.0, 3, 3) == ((3, 3, 3, 3), 1.0)                     # lam 1: an empty box
    box, eff = cutmix_box(10, 20, 0.0, 0, 0)                                        # lam 0 in the corner: clipped to a quarter
    assert box == (0, 0, 5, 10) and eff == 0.75
    rng = random.Random(4)
    for _ in range(300):
        h, w = rng.randrange(1, 300), rng.randrange(1, 300)
        lam, cy, cx = rng.random(), rng.randrange(h), rng.randrange(w)
        (y0, x0, y1, x1), eff = cutmix_box(h, w, lam, cy, cx)
        assert ((y0, x0, y1, x1), eff) == R.box_of(h, w, lam, cy, cx)
        assert 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w
        assert eff == 1.0 - (y1 - y0) * (x1 - x0) / float(h * w) and lam - 1e-12 <= eff <= 1.0     # clipping only shrinks the box


@pytest.mark.parametrize("kw", [dict(mixup_alpha=0.2), dict(cutmix_alpha=1.0), dict(mixup_alpha=0.8, cutmix_alpha=1.0),
                                dict(mixup_alpha=0.8, cutmix_alpha=1.0, per_sample=True),
                                dict(mixup_alpha=0.8, cutmix_alpha=1.0, per_sample=True, prob=0.5, switch_prob=0.3),
                                dict(cutmix_alpha=0.5, prob=0.5), dict()])
def test_describe_matches_restatement(kw):
    from mnasnet_pytorch_amd import DeviceMix
    from mnasnet_pytorch_amd import _lib as L
    assert (L.IMGM_NONE, L.IMGM_MIXUP, L.IMGM_CUTMIX) == (R.NONE, R.MIXUP, R.CUTMIX)
    mix = DeviceMix(**kw)
    modes = set()
    for seed in range(12):
        for n, h, w in [(8, 64, 48), (5, 17, 33), (1, 1, 1), (0, 8, 8)]:
            random.seed(seed)
            got = mix.describe(n, h, w)
            after = random.random()
            random.seed(seed)
            want = R.describe(n, h, w, **kw)
            assert after == random.random()                     # the same number of draws consumed
            assert [tuple(d) for d in got] == want
            assert len(got) == n
            for k, d in enumerate(got):
                modes.add(d.mode)
                assert 0 <= d.partner < max(n, 1) and 0.0 <= d.lam <= 1.0
                if d.mode == R.NONE:
                    assert d.partner == k and d.lam == 1.0
                elif d.mode == R.MIXUP:
                    assert d.lam == d.w16 / 65536.0 and 0 <= d.w16 <= 65536
                else:
                    y0, x0, y1, x1 = d.box
                    assert d.lam == 1.0 - (y1 - y0) * (x1 - x0) / float(h * w)
            if n and not kw.get("per_sample"):
                assert len({(d.mode, d.w16, d.box, d.lam) for d in got}) == 1          # one draw for the whole batch
            if n and all(d.mode != R.NONE for d in got):
                assert sorted(d.partner for d in got) == list(range(n))                # the partners are a permutation
    want_modes = {R.NONE} if not kw or kw.get("prob", 1.0) < 1.0 else set()
    if kw.get("mixup_alpha"):
        want_modes.add(R.MIXUP)
    if kw.get("cutmix_alpha"):
        want_modes.add(R.CUTMIX)
    assert modes == want_modes
    with pytest.raises(ValueError):
        DeviceMix(mixup_alpha=-1.0)
    with pytest.raises(ValueError):
        DeviceMix(prob=1.5)


def _item(L, mode=0, partner=0, w16=0, y0=0, x0=0, y1=0, x1=0, reserved=0):
    return L.MnasImgMix(mode, partner, w16, y0, x0, y1, x1, reserved)


def test_host_check_accepts_and_refuses():
    from mnasnet_pytorch_amd import _lib as L
    lib = L.load()
    assert ctypes.sizeof(L.MnasImgMix) == 32
    n, H, W = 4, 6, 9

    def check(items, n_=n, h=H, w=W):
        arr = (L.MnasImgMix * max(1, len(items)))(*items)
        return lib.mnas_img_mix_check(arr, n_, h, w)

    ok = [_item(L), _item(L, 1, 3, 65536), _item(L, 1, 0, 0), _item(L, 2, 2, 0, 0, 0, 6, 9), _item(L, 2, 1, 12345, 6, 9, 6, 9),
          _item(L, 2, 3, 1, 2, 3, 2, 3), _item(L, 0, 3, 65536, 1, 1, 5, 8)]
    for it in ok:
        assert check([it] * n) == 0
    assert check([], 0) == 0
    bad = [_item(L, 3), _item(L, -1), _item(L, 1, 4), _item(L, 1, -1), _item(L, 1, 0, 65537), _item(L, 1, 0, -1),
           _item(L, 2, 0, 0, 3, 0, 2, 0), _item(L, 2, 0, 0, 0, 5, 0, 4), _item(L, 2, 0, 0, -1, 0, 2, 2), _item(L, 2, 0, 0, 0, -1, 2, 2),
           _item(L, 2, 0, 0, 0, 0, 7, 2), _item(L, 2, 0, 0, 0, 0, 2, 10), _item(L, 0, 0, 0, 0, 0, 0, 0, 1),
           _item(L, 0, 0, 0, 0, 0, 7, 0)]                      # every field is checked whatever the mode
    for it in bad:
        assert check([it] * n) == L.EINVAL, tuple(getattr(it, f) for f, _ in it._fields_)
        assert check([ok[1], ok[3], it, ok[0]]) == L.EINVAL     # one refused item refuses the batch
    assert check([ok[0]] * n, n, 0, W) == L.EINVAL and check([ok[0]] * n, n, H, 16385) == L.EINVAL and check([ok[0]], -1) == L.EINVAL
    assert lib.mnas_img_mix_check(None, 2, H, W) == L.EINVAL
    # the launch wrapper refuses a bad shape before it looks at a pointer
    assert lib.mnas_img_mix(None, 1, 0, 4, None, None, None) == L.EINVAL


def test_python_surface_refuses_cpu_tensors():
    import mnasnet_pytorch_amd as P
    for name in ("MixCrossEntropyLoss", "DeviceMix", "MixedTarget"):
        assert name in P.__all__ and hasattr(P, name)
    crit = P.MixCrossEntropyLoss(label_smoothing=0.1)
    assert isinstance(crit, torch.nn.Module) and crit.label_smoothing == 0.1 and crit.ignore_index == -100
    t = torch.tensor([1, 2])
    with pytest.raises(RuntimeError):
        crit(torch.zeros(2, 5), t)
    mt = P.MixedTarget(t, t.clone(), torch.tensor([0.25, 0.75]))
    assert mt.device.type == "cpu" and len(mt) == 2 and torch.equal(mt.dominant(), t)
    assert torch.equal(P.MixedTarget(t, t + 1, torch.tensor([0.5, 0.49])).dominant(), torch.tensor([1, 3]))
    with pytest.raises(RuntimeError):
        crit(torch.zeros(2, 5), mt)
    with pytest.raises(RuntimeError):
        mt.check_device("cuda:0")
    with pytest.raises(ValueError):
        P.MixCrossEntropyLoss(label_smoothing=1.5)
    with pytest.raises(TypeError):
        P.MixedTarget(t, t.float(), torch.tensor([0.25, 0.75]))
    with pytest.raises(ValueError):
        P.MixedTarget(t, t, torch.tensor([0.25]))
    x = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        P.DeviceMix(mixup_alpha=0.2)(x, t)
    with pytest.raises(RuntimeError):
        P.DeviceMix.apply(x, t, P.DeviceMix(cutmix_alpha=1.0).describe(2, 4, 4))


def test_mixed_target_with_a_foreign_criterion_raises():
    import mnasnet_pytorch_amd as P
    from mnasnet_pytorch_amd.train_step import Trainer
    t = torch.tensor([1, 2])
    mt = P.MixedTarget(t, t.clone(), torch.tensor([0.25, 0.75]))

    class Mine(P.MixCrossEntropyLoss):
        pass

    for c in (torch.nn.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(label_smoothing=0.1), P.MultiClassBCELoss()):
        with pytest.raises(TypeError):
            Trainer._check_target(types.SimpleNamespace(criterion=c), mt)
        Trainer._check_target(types.SimpleNamespace(criterion=c), t)
    for c in (P.MixCrossEntropyLoss(), Mine()):
        Trainer._check_target(types.SimpleNamespace(criterion=c), mt)
    # only the class itself is routed natively; nn.CrossEntropyLoss routes as before
    assert Trainer._mixce(types.SimpleNamespace(criterion=P.MixCrossEntropyLoss(0.1)))
    assert not Trainer._mixce(types.SimpleNamespace(criterion=Mine()))
    assert not Trainer._mixce(types.SimpleNamespace(criterion=torch.nn.CrossEntropyLoss(label_smoothing=0.1)))
    # MultiLabelMeters count label matrices: refused with this criterion (no GPU here, so a stand-in of that class)
    from mnasnet_pytorch_amd.metrics import MultiLabelMeters
    ml = object.__new__(MultiLabelMeters)
    for c in (P.MixCrossEntropyLoss(), Mine()):
        with pytest.raises(ValueError):
            Trainer._check_meters(types.SimpleNamespace(criterion=c), ml)
        Trainer._check_meters(types.SimpleNamespace(criterion=c), None)
