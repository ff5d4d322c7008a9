"""-m gpu: the training step under losses.MultiLabelLoss -- FineTuneModelPool, head '512', 10 classes, 4 x 3 x 64 x 64, no dropout
(the model test_gpu_multilabel.py::test_trainer_step_native_bce builds).  The native step against the module path, the plain
configuration against MultiClassBCELoss bit for bit, DeviceMix on a label matrix, device-mixed against host-mixed labels, the meters
on both paths, validate(), and the refusals."""
import random

import numpy as np
import pytest
import torch

import cases as C
import mix_ref as MR
import mlabel_ex_ref as X
import multilabel_ref as R
from gpu_util import relerr
from mnasnet_pytorch_amd import (DeviceMix, MixCrossEntropyLoss, MixedLabels, MultiClassBCELoss, MultiLabelLoss, MultiLabelMeters)
from mnasnet_pytorch_amd.mixing import MixDraw, cutmix_box
from mnasnet_pytorch_amd.train_step import Trainer

pytestmark = pytest.mark.gpu
POS_WEIGHT = torch.tensor([1.0, 2.0, 0.5, 3.0, 1.5, 1.0, 4.0, 0.75, 2.5, 1.25])
RECIPE = dict(gamma_pos=1, gamma_neg=4, margin=0.05, label_smoothing=0.1)


def _labels(N, classes=10, shift=0):
    return (((torch.arange(N)[:, None] * 3 + torch.arange(classes)[None, :] + shift) % 4) == 0).float()


def _recipe():
    return MultiLabelLoss(pos_weight=POS_WEIGHT, **RECIPE).cuda()


def _mixed(n=4):
    Y = _labels(n)
    return MixedLabels(Y, torch.arange(n).roll(1), torch.tensor([0.3, 0.5, 1.0, 0.0, 0.75, 0.25, 0.6, 0.45][:n])).to("cuda")


def _model(u8=False):
    from test_gpu_train import _no_dropout, build
    torch.manual_seed(11)
    m = build("512", proj_gamma=0.1).train()
    _no_dropout(m)
    if u8:
        m.normalize_on_device()
    return m


def _rule(logits, target, crit, N):
    """the fp64 rule on a step's logits for the RECIPE criterion"""
    pa, la = (target.partner.cpu().numpy(), target.lam.cpu().numpy()) if isinstance(target, MixedLabels) else (None, None)
    Y = (target.labels if isinstance(target, MixedLabels) else target).cpu().numpy()
    return X.loss_and_grad(logits.cpu().numpy(), Y, None, POS_WEIGHT.numpy(), crit.gamma_pos, crit.gamma_neg, crit.margin,
                           crit.label_smoothing, partner=pa, lam=la)


def test_native_step_matches_module_path():
    """two steps of the recipe on a MixedLabels: the native step against model(x) / criterion / backward, with the bounds of
    test_gpu_mix.py::test_mixed_native_step_matches_module_path; the fp64 rule on the native step's logits gives its loss"""
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = _mixed()
    res = []
    for native in (True, False):
        tr = Trainer(_model(), lr=1e-3, criterion=_recipe())
        tr.native_step = native
        assert (tr._native_head() is not None) == native
        losses = [float(tr.step(x, t)) for _ in range(2)]
        res.append((losses, tr.flat_p.clone()))
        if native:
            assert tr.last_logits is not None and tr.last_logits.shape == (4, 10)
            ref = _rule(tr.last_logits, t, tr.criterion, 4)[0]
            assert abs(losses[1] - ref) <= 2e-5 * abs(ref)
    print("losses native %r module %r relerr(params) %.3e" % (res[0][0], res[1][0], relerr(res[0][1].cpu(), res[1][1].cpu())))
    assert np.allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert relerr(res[0][1].cpu(), res[1][1].cpu()) < 1e-5

    class Doubled(MultiLabelLoss):                            # a subclass keeps the module path
        def forward(self, outputs, targets, weights=None):
            return super().forward(outputs, targets, weights) * 2

    tr = Trainer(_model(), lr=1e-3, criterion=Doubled(**RECIPE))
    assert tr._native_head() is None
    l2 = float(tr.step(x, t))
    assert tr.last_logits is None and l2 > 0


def test_plain_configuration_steps_like_multiclass_bce():
    """MultiLabelLoss() steps bit for bit as MultiClassBCELoss() does, with meters"""
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = _labels(4).cuda()
    res = []
    for crit in (MultiLabelLoss(), MultiClassBCELoss()):
        meters = MultiLabelMeters()
        tr = Trainer(_model(), lr=1e-3, criterion=crit, meters=meters)
        assert tr._native_head() is not None
        losses = [tr.step(x, t).clone() for _ in range(2)]
        res.append((losses, tr.flat_p.clone(), meters.block.clone()))
    assert torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0]))
    assert torch.equal(res[0][2], res[1][2])


def _draws():
    box, eff = cutmix_box(64, 64, 0.6, 20, 50)
    return [MixDraw(MR.MIXUP, 2, 12345, (0, 0, 0, 0), 12345 / 65536.0), MixDraw(MR.CUTMIX, 3, 65536, box, eff),
            MixDraw(MR.NONE, 2, 65536, (0, 0, 0, 0), 1.0), MixDraw(MR.MIXUP, 0, 50000, (0, 0, 0, 0), 50000 / 65536.0)]


def test_device_mix_on_a_label_matrix():
    """DeviceMix on a floating (N, C) target: the bytes of mix_ref.mix_batch and a MixedLabels whose partner / lam are the draws';
    the draw order is the class-vector call's; int64 (N,) targets still give a MixedTarget"""
    from mnasnet_pytorch_amd import MixedTarget
    rng = np.random.default_rng(81)
    x = rng.integers(0, 256, (6, 3, 40, 56), dtype=np.uint8)
    Y = _labels(6)
    mix = DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, per_sample=True)
    random.seed(5)
    draws = mix.describe(6, 40, 56)
    random.seed(5)
    xm, ml = mix(torch.from_numpy(x).cuda(), Y.cuda())
    state = random.getstate()
    assert isinstance(ml, MixedLabels) and xm.dtype == torch.uint8 and xm.shape == (6, 3, 40, 56)
    assert np.array_equal(xm.cpu().numpy(), MR.mix_batch(x, [tuple(d) for d in draws]))
    assert torch.equal(ml.labels.cpu(), Y)
    assert torch.equal(ml.partner.cpu(), torch.tensor([d.partner for d in draws]))
    assert torch.equal(ml.lam.cpu(), torch.tensor([d.lam for d in draws], dtype=torch.float32))
    random.seed(5)
    xm2, mt = mix(torch.from_numpy(x).cuda(), torch.arange(6).cuda())
    assert isinstance(mt, MixedTarget) and torch.equal(xm2, xm) and random.getstate() == state
    xm3, ml3 = DeviceMix.apply(torch.from_numpy(x).cuda(), Y.cuda().double(), draws)       # any floating matrix: .float()
    assert ml3.labels.dtype == torch.float32 and torch.equal(xm3, xm)
    with pytest.raises(ValueError):
        DeviceMix.apply(torch.from_numpy(x).cuda(), Y[:5].cuda(), draws)
    with pytest.raises(ValueError):
        DeviceMix.apply(torch.from_numpy(x).cuda(), Y.cuda().long(), draws)


def test_step_on_device_mixed_labels_bit_equal_to_host_mixed():
    """a uint8 batch and a label matrix mixed by DeviceMix.apply from explicit draws, then stepped, against the same step on the
    batch the restatement mixed on the host and a MixedLabels built there: same bytes, bit-equal loss and parameters"""
    rng = np.random.default_rng(80)
    x = rng.integers(0, 256, (4, 3, 64, 64), dtype=np.uint8)
    Y = _labels(4)
    draws = _draws()
    res = []
    for route in ("device", "host"):
        if route == "device":
            xm, ml = DeviceMix.apply(torch.from_numpy(x).cuda(), Y.cuda(), draws)
        else:
            xm = torch.from_numpy(MR.mix_batch(x, [tuple(d) for d in draws])).cuda()
            ml = MixedLabels(Y, torch.tensor([d.partner for d in draws]), torch.tensor([d.lam for d in draws], dtype=torch.float32)).to("cuda")
        tr = Trainer(_model(u8=True), lr=1e-3, criterion=_recipe())
        assert tr._native_head() is not None
        loss = tr.step(xm, ml)
        torch.cuda.synchronize()
        res.append((xm.cpu(), loss.clone(), tr.flat_p.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]) and bool(torch.isfinite(res[0][1]))
    assert torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("native", [True, False])
def test_meters_on_mixed_steps_count_the_dominant_image(native):
    """MultiLabelMeters fed by the mixed step -- inside the loss kernels on the native path, by meters.update on the module path --
    equal the restatement applied to each step's logits, its dominant label rows and its loss; weights N, N and input.size(1)"""
    xs = [C.det_input((8, 3, 64, 64), seed=C.INPUT_SEED + i).cuda() for i in range(2)]
    t = _mixed(8)
    meters = MultiLabelMeters()
    m = _model()
    tr = Trainer(m, lr=1e-3, criterion=_recipe(), meters=meters)
    tr.native_step = native
    assert (tr._native_head() is not None) == native
    logits = []
    hook = m.register_forward_hook(lambda mod, inp, o: logits.append(o.detach().clone()))
    log = R.StepLog()
    dom = t.dominant().cpu().numpy()
    assert np.array_equal(dom, X.dominant(t.labels.cpu().numpy(), t.partner.cpu().numpy(), t.lam.cpu().numpy()))
    for x in xs:
        loss = tr.step(x, t)
        z = (tr.last_logits if native else logits[-1]).cpu().numpy()
        log.update(z, dom, loss.item(), R.hard_dice(z, dom), R.f1_batch(z, dom), 8, 8, 3)
    hook.remove()
    rec = meters.read()
    print(native, rec)
    assert abs(rec.hdice.val - log.hdice.val) <= 4 * 2.0 ** -24
    assert (rec.steps, rec.samples, rec.loss_n, rec.hdice_n, rec.f1_n, rec.nonfinite_steps) == (2, 16, 16, 16, 6, 0)
    assert (rec.tp, rec.fp, rec.fn) == (log.tp, log.fp, log.fn) and (rec.last_tp, rec.last_fp, rec.last_fn) == log.last
    assert rec.f1.val == log.f1.val and rec.f1.avg == log.f1.avg and rec.loss.val == log.loss.val and rec.loss.avg == log.loss.avg


def test_validate_equals_hand_loop_with_one_sync(monkeypatch):
    """validate() under the recipe: the native eval head and mnas_mlabel_loss on plain label matrices; counts and F1 those of a
    hand-written loop, the loss within 2e-5 of the fp64 rule per batch, and no synchronising call before read()"""
    torch.manual_seed(3)
    from test_gpu_train import build
    m = build("512", proj_gamma=0.1).train()               # dropout stays at 0.5: eval mode must switch it off
    tr = Trainer(m, lr=1e-3, criterion=_recipe())
    assert tr._native_eval_head() is not None
    tr.step(C.det_input((8, 3, 64, 64)).cuda(), _labels(8).cuda())
    batches = [(C.det_input((8, 3, H, W), seed=C.INPUT_SEED + 40 + i).cuda(), _labels(8, shift=i).cuda())
               for i, (H, W) in enumerate([(64, 64), (64, 96)])]
    log = R.StepLog()
    m.eval()
    with torch.no_grad():
        for x, t in batches:
            out, tt = m(x).cpu(), t.cpu().numpy()
            loss = _rule(out, t, tr.criterion, 8)[0]
            log.update(out.numpy(), tt, loss, R.hard_dice(out.numpy(), tt), R.f1_batch(out.numpy(), tt), 8, 8, 3)
    m.train()
    tr.validate(batches)                                    # programs of both shapes exist from here on
    count = {"n": 0, "in_read": False}
    real_read = MultiLabelMeters.read

    def read(self):
        count["in_read"] = True
        try:
            return real_read(self)
        finally:
            count["in_read"] = False

    def counting(fn):
        def wrapped(*a, **k):
            if not count["in_read"]:
                count["n"] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(MultiLabelMeters, "read", read)
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counting(getattr(torch.Tensor, name)))
    monkeypatch.setattr(torch.cuda, "synchronize", counting(torch.cuda.synchronize))
    try:
        rec = tr.validate(batches)
    finally:
        monkeypatch.undo()
    assert count["n"] == 0, "validate() took %d synchronising calls before read()" % count["n"]
    assert m.training
    assert (rec.steps, rec.samples, rec.loss_n, rec.hdice_n, rec.f1_n, rec.nonfinite_steps) == (2, 16, 16, 16, 6, 0)
    assert (rec.tp, rec.fp, rec.fn) == (log.tp, log.fp, log.fn) and (rec.last_tp, rec.last_fp, rec.last_fn) == log.last
    assert rec.f1.val == log.f1.val and rec.f1.avg == log.f1.avg
    assert abs(rec.loss.val - log.loss.val) <= 2e-5 * abs(log.loss.val) and abs(rec.loss.avg - log.loss.avg) <= 2e-5 * abs(log.loss.avg)


def test_refusals_leave_the_step_untouched():
    """a MixedLabels handed to MultiClassBCELoss or to a cross-entropy criterion, and a MixedTarget handed to MultiLabelLoss, are
    refused before anything is launched: flat_p and step_count are unchanged; so are meters of the wrong kind"""
    from mnasnet_pytorch_amd import DeviceMeters
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = _mixed()
    m = _model()
    tr = Trainer(m, lr=1e-3, criterion=_recipe())
    before = tr.flat_p.clone()
    for crit in (MultiClassBCELoss(), torch.nn.CrossEntropyLoss(), MixCrossEntropyLoss(0.1)):
        for native in (True, False):
            tr.criterion, tr.native_step = crit, native      # (plain attributes, checked by every step)
            with pytest.raises(TypeError):
                tr.step(x, t)
            assert torch.equal(tr.flat_p, before) and tr.step_count == 0
    tr.criterion, tr.native_step = _recipe(), True
    from test_gpu_mix import _mixed as mixed_target
    with pytest.raises(TypeError):
        tr.step(x, mixed_target())
    with pytest.raises(ValueError):
        Trainer(m, lr=1e-3, criterion=_recipe(), meters=DeviceMeters((1,)))
    tr.meters = DeviceMeters((1,))
    with pytest.raises(ValueError):
        tr.step(x, t)
    assert torch.equal(tr.flat_p, before) and tr.step_count == 0
