"""CPU (no GPU needed): the multi-label loss -- MultiLabelLoss, MixedLabels, mnas_mlabel_loss (include/mnas.h "multi-label loss").
The fp64 restatement (mlabel_ex_ref.py) against torch's BCE-with-logits and against autograd of the formula, the symbol and its
struct, every host-side refusal, the routing, the Python surface, and a bracket that rejects an injected error."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import bounds_mlabel_ex as B
import mlabel_ex_ref as R
from bounds_mlabel import mlabel_inputs
from intervals import check_interval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_torch_bce_with_logits():
    """gamma = 0, m = 0: the sum is F.binary_cross_entropy_with_logits(weight=, pos_weight=) in fp64, both reductions"""
    for (N, C) in ((4, 7), (12, 90)):
        z, Y, w, pw, _, _ = R.batch(N, C)
        for Yv in (Y, R.batch(N, C, soft=True)[1]):
            for wv, pv in ((None, None), (w, None), (None, pw), (w, pw)):
                want = torch.nn.functional.binary_cross_entropy_with_logits(
                    z.double(), Yv.double(), weight=None if wv is None else wv.double(), pos_weight=None if pv is None else pv.double(),
                    reduction="sum")
                for red, D in (("mean", N * C), ("rows", N)):
                    got, _, _ = R.loss_and_grad(z.numpy(), Yv.numpy(), None if wv is None else wv.numpy(),
                                                None if pv is None else pv.numpy(), reduction=red)
                    assert abs(got - float(want) / D) <= 1e-12 * max(1.0, abs(got)), (N, C, red)


@pytest.mark.parametrize("cfg", R.CONFIGS)
def test_closed_form_gradient_equals_autograd(cfg):
    """the closed-form gradient against fp64 autograd of the formula as the issue states it, with mixed labels, pos_weight and
    weights; the batch holds elements on both sides of the margin (sigma <= m: the negative part and its gradient are 0)"""
    gp, gn, m, eps = cfg
    N, C = 6, 37
    z, Y, w, pw, partner, lam = R.batch(N, C, seed=3)
    z = z * 1.5
    if m > 0.0:
        s = torch.sigmoid(z.double())
        assert bool((s <= m).any()) and bool((s > m).any())
    for mix in (False, True):
        for red in ("mean", "rows"):
            kw = dict(gamma_pos=gp, gamma_neg=gn, margin=m, smoothing=eps, reduction=red)
            pa, la = (partner, lam) if mix else (None, None)
            loss, g, _ = R.loss_and_grad(z.numpy(), Y.numpy(), w.numpy(), pw.numpy(), partner=None if pa is None else pa.numpy(),
                                         lam=None if la is None else la.numpy(), **kw)
            zt = z.double().clone().requires_grad_(True)
            lt = R.formula_torch(zt, Y.double(), w.double(), pw.double(), partner=pa, lam=None if la is None else la.double(), **kw)
            lt.backward()
            assert abs(loss - float(lt.detach())) <= 1e-13 * max(1.0, abs(loss))
            assert float((torch.tensor(g) - zt.grad).abs().max()) <= 1e-14, (cfg, mix, red)
            dead = torch.sigmoid(z.double()) <= m
            if m > 0.0 and not mix and eps == 0.0:          # a pure negative beyond the margin: no loss, no gradient
                sel = dead & (Y == 0)
                assert bool(sel.any()) and bool((torch.tensor(g)[sel] == 0).all())


def test_symbol_struct_and_version():
    from mnasnet_pytorch_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mnas.h")).read()
    assert re.search(r"\bint mnas_mlabel_loss\(", hdr)
    assert "mnas_mlabel_loss" in _lib.SYMBOLS and hasattr(lib, "mnas_mlabel_loss")
    assert len(_lib.SYMBOLS["mnas_mlabel_loss"][1]) == 17
    assert lib.mnas_version() == _lib.ABI_VERSION == 8                    # additive
    assert ctypes.sizeof(_lib.MnasMlabelLoss) == 32
    body = re.search(r"typedef struct MnasMlabelLoss \{(.*?)\} MnasMlabelLoss;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?\s*[,;]", body) == [n for n, _ in _lib.MnasMlabelLoss._fields_]
    macro = {k: int(v) for k, v in re.findall(r"#define (MNAS_MLABEL_(?:MEAN|ROWS))\s+(\d+)", hdr)}
    assert (macro["MNAS_MLABEL_MEAN"], macro["MNAS_MLABEL_ROWS"]) == (_lib.MLABEL_MEAN, _lib.MLABEL_ROWS) == (0, 1)
    # what must not move
    assert len(_lib.SYMBOLS["mnas_mlabel_bce"][1]) == 16 and len(_lib.SYMBOLS["mnas_mlabel_metrics"][1]) == 11
    assert len(_lib.SYMBOLS["mnas_mlabel_hard_dice"][1]) == 9
    assert lib.mnas_mlabel_scratch_bytes(12) == 24 * 12 + 16


def _call(lib, _lib, logits=4096, labels=4096, partner=None, lam=None, weights=None, pw=None, N=4, C=10, cfg=(0.0, 0.0, 0.0, 0.0, 0),
          scratch=4096, loss=4096, dl=None, meters=None, n=(0, 0, 0), null_cfg=False, reserved=0):
    c = _lib.MnasMlabelLoss(cfg[0], cfg[1], cfg[2], cfg[3], cfg[4])
    c.reserved[1] = reserved
    return lib.mnas_mlabel_loss(logits, labels, partner, lam, weights, pw, N, C, None if null_cfg else ctypes.byref(c), scratch, loss, dl,
                                meters, n[0], n[1], n[2], None)


def test_host_refusals():
    """every refusal comes on the host, before any launch (no GPU is touched: all return EINVAL first).  4096 stands for a non-NULL,
    16-byte aligned pointer that is never dereferenced on these paths."""
    from mnasnet_pytorch_amd import _lib
    lib = _lib.load()
    E, p = _lib.EINVAL, 4096
    call = lambda **kw: _call(lib, _lib, **kw)                # noqa: E731
    for name in ("logits", "labels", "scratch", "loss"):      # every NULL pointer
        assert call(**{name: None}) == E, name
    assert call(null_cfg=True) == E
    assert call(N=0) == E and call(C=0) == E and call(N=-1) == E
    nan = float("nan")
    for g in (0.5, -1.0, 16.5, 0.999, nan, float("inf")):     # gamma in {0} u [1, 16]
        assert call(cfg=(g, 0.0, 0.0, 0.0, 0)) == E, g
        assert call(cfg=(0.0, g, 0.0, 0.0, 0)) == E, g
    for m in (-0.01, 0.51, nan, float("inf")):
        assert call(cfg=(0.0, 0.0, m, 0.0, 0)) == E, m
    for eps in (-0.1, 1.0, 1.5, nan):
        assert call(cfg=(0.0, 0.0, 0.0, eps, 0)) == E, eps
    assert call(cfg=(0.0, 0.0, 0.0, 0.0, 2)) == E and call(cfg=(0.0, 0.0, 0.0, 0.0, -1)) == E      # reduction
    assert call(reserved=1) == E
    assert call(lam=p) == E and call(partner=p) == E          # lam without partner, partner without lam
    assert call(scratch=p + 4) == E                           # a misaligned scratch
    for n in ((-1, 4, 4), (4, -1, 4), (4, 4, -1)):            # a negative meter weight
        assert call(meters=p, n=n) == E


def test_routing_and_trainer_checks():
    import mnasnet_pytorch_amd as P
    from mnasnet_pytorch_amd.train_step import Trainer
    NS = types.SimpleNamespace

    class Mine(P.MultiLabelLoss):
        def forward(self, outputs, targets, weights=None):
            return super().forward(outputs, targets, weights) * 2

    assert Trainer._mlloss(NS(criterion=P.MultiLabelLoss()))
    assert not Trainer._mlloss(NS(criterion=Mine()))                            # a subclass keeps the module path
    assert not Trainer._mlloss(NS(criterion=P.MultiClassBCELoss()))
    # _multilabel still answers for MultiClassBCELoss only
    assert Trainer._multilabel(NS(criterion=P.MultiClassBCELoss()))
    assert not Trainer._multilabel(NS(criterion=P.MultiLabelLoss()))
    assert not Trainer._multilabel(NS(criterion=Mine()))
    ml = P.MixedLabels(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), torch.ones(2))
    mt = P.MixedTarget(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.ones(2))
    for c in (P.MultiLabelLoss(), Mine()):
        Trainer._check_target(NS(criterion=c), ml)
        Trainer._check_target(NS(criterion=c), torch.zeros(2, 3))
        with pytest.raises(TypeError):
            Trainer._check_target(NS(criterion=c), mt)                          # a MixedTarget is the single-label branch's
        with pytest.raises(ValueError):
            Trainer._check_meters(NS(criterion=c), object())
        with pytest.raises(ValueError):
            Trainer._check_meters(NS(criterion=c), P.DeviceMeters.__new__(P.DeviceMeters))
        Trainer._check_meters(NS(criterion=c), None)
        Trainer._check_meters(NS(criterion=c), P.MultiLabelMeters.__new__(P.MultiLabelMeters))
    for c in (P.MultiClassBCELoss(), torch.nn.CrossEntropyLoss(), P.MixCrossEntropyLoss(), P.DistillCrossEntropyLoss()):
        with pytest.raises(TypeError):
            Trainer._check_target(NS(criterion=c), ml)


def test_python_surface():
    import mnasnet_pytorch_amd as P
    from mnasnet_pytorch_amd import losses
    from mnasnet_pytorch_amd.head import NativeHead
    for name in ("MultiLabelLoss", "MixedLabels"):
        assert name in P.__all__ and hasattr(P, name)
    sig = inspect.signature(P.MultiLabelLoss.__init__).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [
        ("gamma_pos", 0.0), ("gamma_neg", 0.0), ("margin", 0.0), ("pos_weight", None), ("label_smoothing", 0.0),
        ("use_weight_mask", False), ("reduction", "mean")]
    sig = inspect.signature(P.MultiLabelLoss.forward).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("outputs", inspect.Parameter.empty), ("targets", inspect.Parameter.empty),
                                                                  ("weights", None)]
    assert callable(losses.multilabel_loss) and callable(NativeHead.mlabel)
    assert list(inspect.signature(P.MixedLabels.__init__).parameters)[1:] == ["labels", "partner", "lam"]
    # pos_weight is a registered buffer
    c = P.MultiLabelLoss(1, 4, 0.05, pos_weight=torch.tensor([1.0, 2.0, 3.0]), label_smoothing=0.1)
    assert "pos_weight" in dict(c.named_buffers()) and c.pos_weight.dtype == torch.float32
    assert "pos_weight" in dict(P.MultiLabelLoss().named_buffers(recurse=False)) or P.MultiLabelLoss().pos_weight is None
    # the ranges the kernel refuses are ValueErrors here
    for kw in (dict(gamma_pos=0.5), dict(gamma_neg=17), dict(gamma_neg=float("nan")), dict(margin=0.6), dict(margin=-0.1),
               dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(reduction="sum"), dict(pos_weight=torch.tensor([-1.0])),
               dict(pos_weight=torch.ones(2, 2))):
        with pytest.raises(ValueError):
            P.MultiLabelLoss(**kw)
    # MultiClassBCELoss keeps its constructor
    sig = inspect.signature(P.MultiClassBCELoss.__init__).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("use_weight_mask", False), ("use_focal_weights", False),
                                                                  ("focus_param", 2), ("balance_param", 0.25)]
    sig = inspect.signature(P.MultiLabelMeters.update).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("logits", inspect.Parameter.empty), ("target", inspect.Parameter.empty),
                                                                  ("loss", None), ("f1_n", None)]


def test_mixed_labels_checks_and_views():
    import mnasnet_pytorch_amd as P
    Y = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    partner, lam = torch.tensor([2, 0, 1]), torch.tensor([0.25, 0.5, 1.0])
    ml = P.MixedLabels(Y, partner, lam)
    assert len(ml) == 3 and ml.shape == (3, 3) and ml.device.type == "cpu" and "MixedLabels" in repr(ml)
    assert torch.equal(ml.dominant(), torch.stack([Y[2], Y[1], Y[2]]))          # lam >= 0.5 keeps the row itself
    assert torch.equal(ml.dense(), lam[:, None] * Y + (1 - lam[:, None]) * Y[partner])
    assert isinstance(ml.to("cpu"), P.MixedLabels)
    with pytest.raises(RuntimeError):
        ml.check_device("cuda:0")                                               # no CPU path
    for bad in ((Y.double(), partner, lam), (Y, partner.int(), lam), (Y, partner, lam.double()), (Y[0], partner, lam),
                (Y, partner[:, None], lam), ("x", partner, lam)):
        with pytest.raises(TypeError):
            P.MixedLabels(*bad)
    for bad in ((Y, partner[:2], lam), (Y, partner, lam[:2]), (Y[:2], partner, lam)):
        with pytest.raises(ValueError):
            P.MixedLabels(*bad)


def test_no_cpu_path():
    import mnasnet_pytorch_amd as P
    from mnasnet_pytorch_amd import losses
    z, Y = torch.zeros(2, 3), torch.zeros(2, 3)
    with pytest.raises(RuntimeError):
        P.MultiLabelLoss()(z, Y)
    with pytest.raises(RuntimeError):
        P.MultiLabelLoss(1, 4, 0.05)(z, P.MixedLabels(Y, torch.zeros(2, dtype=torch.int64), torch.ones(2)))
    with pytest.raises(RuntimeError):
        losses.multilabel_loss(z, Y)
    with pytest.raises(RuntimeError):
        P.DeviceMix(mixup_alpha=0.2)(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), Y)
    with pytest.raises(RuntimeError):
        P.DeviceMix.apply(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), Y, [])


@pytest.mark.parametrize("cfg", B.EX_CONFIGS)
def test_bracket_holds_the_rule_and_rejects_an_injected_error(cfg):
    """the fp64 value of the rule, rounded once, lies inside every element's bracket on every input kind (with mixed rows); the
    same tensor with ONE element moved by 2^-17 of its magnitude is refused"""
    N, C = 5, 257
    _, _, _, pw, partner, lam = R.batch(N, C)
    pwv = pw if cfg[4] else None
    for kind in ("scale0.5", "scale8", "edges", "soft", "pow2w"):
        z, Y, w = mlabel_inputs(kind, N, C)
        iv = B.mlabel_ex_intervals(z, Y, w, pwv, N, C, cfg[:4], False, partner, lam)
        _, g, e = R.loss_and_grad(z.numpy(), Y.numpy(), w.numpy(), None if pwv is None else pwv.numpy(), *cfg[:4],
                                  partner=partner.numpy(), lam=lam.numpy())
        g32 = torch.tensor(g).float()
        check_interval(g32, iv["dl"], "dlogits", None)
        e64 = torch.tensor(e)
        assert bool(((e64 >= iv["ew"].lo) & (e64 <= iv["ew"].hi)).all())
        k = int(g32.abs().reshape(-1).argmax())
        bad = g32.clone().reshape(-1)
        bad[k] = bad[k] * (1.0 + 2.0 ** -17)
        with pytest.raises(AssertionError):
            check_interval(bad.view(N, C), iv["dl"], "dlogits", None)
    assert np.isfinite(g).all()
