"""CPU (no GPU needed): the fp64 restatement of the distillation cross-entropy (tests/kd_ref.py) against torch's own composition and
against autograd; the C prototype in the header and in _lib; what the Python surface refuses before it touches a device."""
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import kd_ref as K
import mix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def _case(N, C, seed):
    z, t = _rand((N, C), seed) * 4, _rand((N, C), seed + 1) * 6
    i = torch.arange(N)
    y, y2 = (i * 7 + 3) % C, (i * 5 + 1) % C
    lam = torch.tensor([0.0, 0.5, 1.0, 0.3, 0.8125])[i % 5].double()
    return z, t, y, y2, lam


def _weights(C, how):
    if how == "none":
        return None
    w = torch.rand(C, generator=torch.Generator().manual_seed(5), dtype=torch.float64) + 0.25
    if how == "zeros":
        w[::3] = 0.0
    return w


def _torch_loss(z, y, w, eps, t, T, alpha, ignore_index=-100):
    """the composition a user would write in ATen"""
    hard = F.cross_entropy(z, y, weight=w, label_smoothing=eps, ignore_index=ignore_index)
    if t is None or alpha == 0.0:
        return hard, hard, None
    kd = T * T * F.kl_div(F.log_softmax(z / T, 1), F.softmax(t / T, 1), reduction="batchmean")
    return (kd if alpha == 1.0 else (1.0 - alpha) * hard + alpha * kd), hard, kd


@pytest.mark.parametrize("how", ["none", "positive", "zeros"])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.3])
@pytest.mark.parametrize("T,alpha", [(1.0, 0.0), (2.0, 0.5), (4.5, 1.0), (1.0, 0.25)])
def test_restatement_equals_torch_on_plain_targets(how, eps, T, alpha):
    """loss, both parts and the closed-form gradient against F.cross_entropy(weight=, label_smoothing=) + T^2 kl_div(batchmean) and
    autograd, at 1e-12: with ignored rows, weights with zeros and -inf teacher classes"""
    for N, C in [(1, 1), (6, 5), (9, 13)]:
        z, t, y, _, _ = _case(N, C, 10 * N + C)
        w = _weights(C, how)
        if N > 1:
            y = y.clone()
            y[1] = -100                                       # an ignored row: out of the hard term, inside the distillation term
        if C > 2:
            t[:, 1] = float("-inf")                           # a masked teacher class: pT == 0 adds exactly 0
            t[0, 2] = float("-inf")
        zz = z.clone().requires_grad_(True)
        want, hard, kd = _torch_loss(zz, y, w, eps, t, T, alpha)
        if w is not None and float(w[y[y >= 0]].sum()) == 0.0:
            continue                                          # every counted label has weight 0: 0 / 0 on both sides
        want.backward()
        got = K.kd_loss(z, y, eps=eps, w=w, t=t, T=T, alpha=alpha)
        what = (how, eps, T, alpha, N, C)
        assert abs(float(got["loss"]) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach()))), what
        assert abs(float(got["hard"]) - float(hard.detach())) <= 1e-12 * max(1.0, abs(float(hard.detach()))), what
        if kd is not None:
            assert abs(float(got["kd"]) - float(kd.detach())) <= 1e-12 * max(1.0, abs(float(kd.detach()))), what
            assert bool(torch.isfinite(got["kd_rows"]).all()), what
        assert float((got["grad"] - zz.grad).abs().max()) <= 1e-12, what


@pytest.mark.parametrize("how", ["none", "positive", "zeros"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_restatement_equals_torch_on_mixed_targets(how, eps):
    """two labels per row: lam CE_w(a) + (1 - lam) CE_w(b) per row from F.cross_entropy(reduction='none'), divided by the labels'
    weights; the gradient against autograd"""
    N, C, T, alpha = 10, 7, 2.0, 0.5
    z, t, a, b, lam = _case(N, C, 3)
    a = a.clone()
    a[4] = -100
    w = _weights(C, how)
    keep = (a != -100) & (b != -100)
    a0 = torch.where(keep, a, torch.zeros_like(a))
    zz = z.clone().requires_grad_(True)
    rows = lam * F.cross_entropy(zz, a0, weight=w, label_smoothing=eps, reduction="none") + \
        (1 - lam) * F.cross_entropy(zz, b, weight=w, label_smoothing=eps, reduction="none")
    wv = torch.ones(C, dtype=torch.float64) if w is None else w
    D = ((lam * wv[a0] + (1 - lam) * wv[b]) * keep).sum()
    hard = (rows * keep).sum() / D
    kd = T * T * F.kl_div(F.log_softmax(zz / T, 1), F.softmax(t / T, 1), reduction="batchmean")
    want = (1 - alpha) * hard + alpha * kd
    want.backward()
    got = K.kd_loss(z, a, b, lam, eps, w, t, T, alpha)
    assert abs(float(got["loss"]) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    assert abs(float(got["D"]) - float(D)) <= 1e-12
    assert float((got["grad"] - zz.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_unit_weights_and_no_teacher_is_the_soft_cross_entropy(eps):
    N, C = 9, 11
    z, _, a, b, lam = _case(N, C, 4)
    a = a.clone()
    a[2] = -100
    for bb, ll in ((None, None), (b, lam)):
        ref, gref = R.soft_ce(z, a, bb, ll, eps)
        for w in (None, torch.ones(C, dtype=torch.float64)):
            for alpha in (0.0, 0.5):                          # without a teacher alpha does not matter
                got = K.kd_loss(z, a, bb, ll, eps, w, None, 3.0, alpha)
                assert abs(float(got["loss"]) - float(ref)) <= 1e-12
                assert float((got["grad"] - gref).abs().max()) <= 1e-12
                assert float(got["kd"]) == 0.0


def test_edge_rules_of_the_restatement():
    z, t, y, _, _ = _case(4, 6, 8)
    # a -inf student logit under teacher mass: the row's kd is +inf, the closed-form gradient finite
    zi = z.clone()
    zi[1, 3] = float("-inf")
    yi = y.clone()
    yi[1] = 0
    got = K.kd_loss(zi, yi, t=t, T=2.0, alpha=0.5)
    assert float(got["kd_rows"][1]) == float("inf") and bool(torch.isfinite(got["kd_rows"][[0, 2, 3]]).all())
    assert bool(torch.isfinite(got["grad"]).all())
    # every row ignored: hard is NaN, kd finite
    none = torch.full((4,), -100)
    got = K.kd_loss(z, none, t=t, T=2.0, alpha=0.5)
    assert bool(torch.isnan(got["hard"])) and bool(torch.isfinite(got["kd"])) and bool(torch.isnan(got["loss"]))
    got = K.kd_loss(z, none, t=t, T=2.0, alpha=1.0)
    assert bool(torch.isfinite(got["loss"])) and float(got["loss"]) == float(got["kd"])
    # identical teacher and student: kd == 0
    got = K.kd_loss(z, y, t=z.clone(), T=4.5, alpha=1.0)
    assert abs(float(got["kd"])) <= 1e-15


def test_prototype_is_declared_in_header_and_lib():
    from mnasnet_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mnas.h")).read()
    m = re.search(r"\bint mnas_head_cross_entropy_kd\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/mnas.h does not declare mnas_head_cross_entropy_kd"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib.SYMBOLS["mnas_head_cross_entropy_kd"]
    assert len(params) == len(args) == 22 and res is _lib.c_int
    for p, a in zip(params, args):
        if p.startswith("float "):
            assert a is _lib.c_float, p
        elif p.startswith("int64_t "):
            assert a is _lib.c_int64, p
        elif p.startswith("int "):
            assert a is _lib.c_int, p
        else:
            assert "*" in p and a not in (_lib.c_float, _lib.c_int, _lib.c_int64), p
    names = [re.split(r"[ *]", p)[-1] for p in params]
    assert names == ["logits", "target_a", "target_b", "lam", "label_smoothing", "class_weight", "teacher_logits", "temperature", "alpha",
                     "N", "C", "ignore_index", "loss_rows", "loss", "loss_parts", "dlogits", "bad_flag", "ks", "nk", "rank_rows", "meters",
                     "stream"]
    assert _lib.ABI_VERSION == 8
    # the operation order the brackets follow is written next to the kernel
    src = open(os.path.join(ROOT, "mnasnet_pytorch_amd", "csrc", "mnas_head.hip")).read()
    assert "Operation order" in src and "k_head_ce_kd" in src


def test_constructor_refusals():
    import mnasnet_pytorch_amd as P
    for name in ("DistillCrossEntropyLoss", "DistillTarget"):
        assert name in P.__all__ and hasattr(P, name)
    c = P.DistillCrossEntropyLoss()
    assert isinstance(c, torch.nn.Module)
    assert (c.temperature, c.alpha, c.label_smoothing, c.weight, c.ignore_index, c.last_parts) == (1.0, 0.5, 0.0, None, -100, None)
    w = torch.tensor([1.0, 0.0, 2.5])
    c = P.DistillCrossEntropyLoss(2.0, 0.25, 0.1, weight=w, ignore_index=-1)
    assert "weight" in dict(c.named_buffers()) and torch.equal(c.weight, w) and c.weight.dtype == torch.float32
    assert (c.temperature, c.alpha, c.label_smoothing, c.ignore_index) == (2.0, 0.25, 0.1, -1)
    assert torch.equal(P.DistillCrossEntropyLoss(weight=w.double()).weight, w)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(alpha=-0.1), dict(alpha=1.5),
               dict(alpha=float("nan")), dict(label_smoothing=-0.1), dict(label_smoothing=1.5), dict(label_smoothing=float("nan")),
               dict(weight=torch.tensor([1.0, -0.5])), dict(weight=torch.tensor([1.0, float("nan")])),
               dict(weight=torch.tensor([1.0, float("inf")])), dict(weight=torch.ones(2, 3)), dict(weight=torch.tensor(1.0)),
               dict(weight=torch.ones(0)), dict(weight=[1.0, 2.0])):
        with pytest.raises(ValueError):
            P.DistillCrossEntropyLoss(**kw)
    # no CPU path; the class count of the weights is checked against the logits
    with pytest.raises(RuntimeError):
        P.DistillCrossEntropyLoss()(torch.zeros(2, 3), torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        P.DistillCrossEntropyLoss(weight=w).class_weight(torch.zeros(2, 5))


def test_distill_target_device_and_shape_checks():
    import mnasnet_pytorch_amd as P
    y = torch.tensor([1, 2])
    mt = P.MixedTarget(y, y.clone(), torch.tensor([0.25, 0.75]))
    for target in (y, mt):
        dt = P.DistillTarget(target, torch.zeros(2, 5))
        assert dt.device.type == "cpu" and len(dt) == 2 and dt.target is target and tuple(dt.shape) == (2,)
        assert isinstance(dt.to("cpu"), P.DistillTarget)
        with pytest.raises(RuntimeError):
            dt.check_device("cuda:0")
    assert not P.DistillTarget(y, torch.zeros(2, 5, requires_grad=True)).teacher_logits.requires_grad
    with pytest.raises(ValueError):
        P.DistillTarget(y, torch.zeros(3, 5))                 # rows
    for bad in (torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2), torch.zeros(2, 5, 1), [[0.0] * 5] * 2):
        with pytest.raises(TypeError):
            P.DistillTarget(y, bad)
    for bad in (y.float(), y.view(2, 1), [1, 2], P.DistillTarget(y, torch.zeros(2, 5))):
        with pytest.raises(TypeError):
            P.DistillTarget(bad, torch.zeros(2, 5))
    with pytest.raises(RuntimeError):
        P.DistillTarget(y, torch.zeros(2, 5, device="meta"))  # two devices


def test_distill_target_with_a_foreign_criterion_raises():
    import mnasnet_pytorch_amd as P
    from mnasnet_pytorch_amd.train_step import Trainer
    y = torch.tensor([1, 2])
    mt = P.MixedTarget(y, y.clone(), torch.tensor([0.25, 0.75]))

    class Mine(P.DistillCrossEntropyLoss):
        pass

    for target in (P.DistillTarget(y, torch.zeros(2, 5)), P.DistillTarget(mt, torch.zeros(2, 5))):
        for c in (torch.nn.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(weight=torch.ones(5)), P.MixCrossEntropyLoss(0.1),
                  P.MultiClassBCELoss()):
            with pytest.raises(TypeError):
                Trainer._check_target(types.SimpleNamespace(criterion=c), target)
        for c in (P.DistillCrossEntropyLoss(), Mine()):
            Trainer._check_target(types.SimpleNamespace(criterion=c), target)
            Trainer._check_target(types.SimpleNamespace(criterion=c), mt)
            Trainer._check_target(types.SimpleNamespace(criterion=c), y)
    # only the class itself is routed natively; a teacher needs the criterion that takes its logits
    assert Trainer._distill(types.SimpleNamespace(criterion=P.DistillCrossEntropyLoss(2.0)))
    assert not Trainer._distill(types.SimpleNamespace(criterion=Mine()))
    assert not Trainer._distill(types.SimpleNamespace(criterion=P.MixCrossEntropyLoss()))
    teacher = torch.nn.Linear(2, 2)
    with pytest.raises(TypeError):
        Trainer._check_teacher(types.SimpleNamespace(criterion=torch.nn.CrossEntropyLoss(), teacher=teacher))
    with pytest.raises(TypeError):
        Trainer._check_teacher(types.SimpleNamespace(criterion=P.DistillCrossEntropyLoss(), teacher="resnet"))
    Trainer._check_teacher(types.SimpleNamespace(criterion=P.DistillCrossEntropyLoss(), teacher=teacher))
    Trainer._check_teacher(types.SimpleNamespace(criterion=torch.nn.CrossEntropyLoss(), teacher=None))
    # MultiLabelMeters count label matrices: refused with this criterion (no GPU here, so a stand-in of that class)
    from mnasnet_pytorch_amd.metrics import MultiLabelMeters
    ml = object.__new__(MultiLabelMeters)
    with pytest.raises(ValueError):
        Trainer._check_meters(types.SimpleNamespace(criterion=P.DistillCrossEntropyLoss()), ml)
    Trainer._check_meters(types.SimpleNamespace(criterion=P.DistillCrossEntropyLoss()), None)
