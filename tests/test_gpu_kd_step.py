"""-m gpu: Trainer steps under DistillCrossEntropyLoss -- class weights, smoothing, a mixed batch and a teacher's logits in the native
step against the module path; the teacher is left as it was; Trainer(teacher=) against an explicit DistillTarget; validate(); class
weights alone against nn.CrossEntropyLoss(weight=).  Model and input of tests/test_gpu_mix.py."""
import numpy as np
import pytest
import torch

import cases as C
import kd_ref as K
from cases import O
from gpu_util import relerr

pytestmark = pytest.mark.gpu


def _model(seed=None):
    """build("512", proj_gamma=0.1) of test_gpu_train.py, dropout off; seed: other weights (the teacher)"""
    from test_gpu_train import build, _no_dropout
    m = build("512", proj_gamma=0.1)
    if seed is not None:
        m.load_state_dict({**O.init_state(False, seed, proj_gamma=0.1), **O.init_head_state("512", 10, seed)})
    m.train()
    _no_dropout(m)
    return m


def _mixed(n=4):
    from mnasnet_pytorch_amd import MixedTarget
    a = torch.tensor([1, 3, 5, 7, 2, 9, 0, 4][:n])
    return MixedTarget(a, a.roll(1), torch.tensor([0.3, 0.5, 1.0, 0.0, 0.75, 0.25, 0.6, 0.45][:n])).to("cuda")


def _weight():
    return torch.tensor([1.0, 0.5, 2.0, 0.0, 1.5, 0.25, 1.0, 3.0, 0.75, 1.25])


def _state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _same_state(m, before):
    now = m.state_dict()
    return list(now) == list(before) and all(torch.equal(now[k], v) for k, v in before.items())


def test_distilled_native_step_matches_module_path():
    """DistillCrossEntropyLoss(2.0, 0.5, 0.1, weight=w) on a MixedTarget with the teacher given to the Trainer: the native step against
    model(x) / criterion / backward, two steps, with the bounds of test_gpu_mix.py::test_mixed_native_step_matches_module_path; the
    teacher's state_dict bitwise unchanged and its train/eval flags as they were"""
    from mnasnet_pytorch_amd import DistillCrossEntropyLoss
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = _mixed()
    res = []
    for native in (True, False):
        teacher = _model(C.STATE_SEED + 1)
        teacher.features.eval()                               # mixed flags: restored one by one, not with teacher.train()
        flags = [mod.training for mod in teacher.modules()]
        before = _state(teacher)
        crit = DistillCrossEntropyLoss(2.0, 0.5, 0.1, weight=_weight())
        tr = Trainer(_model(), lr=1e-3, criterion=crit, teacher=teacher)
        tr.native_step = native
        losses = [float(tr.step(x, t)) for _ in range(2)]
        parts = crit.last_parts.cpu()
        res.append((losses, tr.flat_p.clone(), parts))
        assert (tr._native_head() is not None) == native
        assert _same_state(teacher, before), "the step wrote to the teacher"
        assert [mod.training for mod in teacher.modules()] == flags and any(flags) and not all(flags)
        assert bool(torch.isfinite(parts).all()) and float(parts[1]) > 0
        assert abs(0.5 * float(parts[0]) + 0.5 * float(parts[1]) - losses[1]) < 1e-5 * max(1.0, abs(losses[1]))
    print("losses native %r module %r relerr(params) %.3e parts %r %r"
          % (res[0][0], res[1][0], relerr(res[0][1].cpu(), res[1][1].cpu()), res[0][2].tolist(), res[1][2].tolist()))
    assert np.allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert relerr(res[0][1].cpu(), res[1][1].cpu()) < 1e-5


def test_teacher_flags_restored_when_the_step_raises():
    from mnasnet_pytorch_amd import DistillCrossEntropyLoss
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input((4, 3, 64, 64)).cuda()
    teacher = _model(C.STATE_SEED + 1)
    teacher.features.eval()
    flags = [mod.training for mod in teacher.modules()]
    before = _state(teacher)
    tr = Trainer(_model(), lr=1e-3, criterion=DistillCrossEntropyLoss(2.0, 0.5), teacher=teacher)
    p0 = tr.flat_p.clone()
    with pytest.raises(RuntimeError):
        tr.step(x, torch.tensor([1, 3, 5, 7]))                # a target left on the host
    assert [mod.training for mod in teacher.modules()] == flags and _same_state(teacher, before)

    def boom(mod, inp, out):
        raise KeyError("teacher forward failed")

    hook = teacher.register_forward_hook(boom)
    with pytest.raises(KeyError):
        tr.step(x, torch.tensor([1, 3, 5, 7]).cuda())         # the teacher's forward raises while it is in eval mode
    hook.remove()
    assert [mod.training for mod in teacher.modules()] == flags and _same_state(teacher, before)
    assert torch.equal(tr.flat_p, p0) and tr.step_count == 0
    # a teacher whose output is not (N, C) fp32 on the batch's device
    tr.teacher = torch.nn.Flatten().cuda()
    with pytest.raises(ValueError):
        tr.step(x.half(), torch.tensor([1, 3, 5, 7]).cuda())
    # a teacher needs the criterion that takes its logits
    with pytest.raises(TypeError):
        Trainer(_model(), lr=1e-3, teacher=teacher)
    assert torch.equal(tr.flat_p, p0) and tr.step_count == 0


def test_trainer_teacher_and_explicit_distill_target_step_bit_equal():
    from mnasnet_pytorch_amd import DistillCrossEntropyLoss, DistillTarget
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = _mixed()
    teacher = _model(C.STATE_SEED + 1).eval()
    with torch.no_grad():
        logits = teacher(x).clone()
    teacher.train()
    res = []
    for explicit in (False, True):
        tr = Trainer(_model(), lr=1e-3, criterion=DistillCrossEntropyLoss(2.0, 0.5, 0.1, weight=_weight()),
                     teacher=None if explicit else teacher)
        assert tr._native_head() is not None
        target = DistillTarget(t, logits) if explicit else t
        losses = [tr.step(x, target).clone() for _ in range(2)]
        res.append((losses, tr.flat_p.clone()))
    assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0])) and bool(torch.isfinite(res[0][0][1]))
    assert torch.equal(res[0][1], res[1][1])


def test_distill_target_for_another_criterion_is_refused_before_anything_is_launched():
    from mnasnet_pytorch_amd import DistillTarget
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input((4, 3, 64, 64)).cuda()
    tr = Trainer(_model(), lr=1e-3)                           # nn.CrossEntropyLoss
    before = tr.flat_p.clone()
    with pytest.raises(TypeError):
        tr.step(x, DistillTarget(torch.tensor([1, 3, 5, 7]).cuda(), torch.zeros(4, 10, device="cuda")))
    assert torch.equal(tr.flat_p, before) and tr.step_count == 0


def test_validate_runs_the_native_eval_head_with_the_hard_term():
    """validate() under DistillCrossEntropyLoss: the native eval head and the kd entry point without a teacher; the loss meter is the
    hard term (weights and smoothing applied) of kd_ref on the logged logits, within 2e-5 max(1, |ref|)"""
    from mnasnet_pytorch_amd import DistillCrossEntropyLoss
    from mnasnet_pytorch_amd.train_step import Trainer
    torch.manual_seed(3)
    m = _model()
    w = _weight()
    tr = Trainer(m, lr=1e-3, criterion=DistillCrossEntropyLoss(2.0, 0.5, 0.1, weight=w), teacher=_model(C.STATE_SEED + 1))
    assert tr._native_eval_head() is not None
    batches = [(C.det_input((8, 3, H, W), seed=C.INPUT_SEED + 40 + i).cuda(), ((torch.arange(8) * 7 + i) % 10).cuda())
               for i, (H, W) in enumerate([(64, 64), (64, 96)])]
    want = []
    m.eval()
    with torch.no_grad():
        for x, t in batches:
            want.append(float(K.kd_loss(m(x).cpu(), t.cpu(), eps=0.1, w=w)["hard"]))
    m.train()
    lib = tr._native_eval_head().lib
    calls = []
    typed = lib.mnas_head_cross_entropy_kd
    lib.mnas_head_cross_entropy_kd = lambda *a: (calls.append(a[6]), typed(*a))[1]
    try:
        rec = tr.validate(batches)
    finally:
        lib.mnas_head_cross_entropy_kd = typed
    avg = sum(want) / 2
    print("validate:", rec, "| kd_ref hard terms %r" % (want,))
    assert calls == [0, 0]                                    # two batches, no teacher logits
    assert (rec.samples, rec.steps) == (16, 2) and m.training
    assert abs(rec.loss.val - want[1]) <= 2e-5 * max(1.0, abs(want[1]))
    assert abs(rec.loss.avg - avg) <= 2e-5 * max(1.0, abs(avg))


def test_class_weights_alone_match_cross_entropy_with_weight():
    """alpha = 0 and a weight on class indices: one native step against nn.CrossEntropyLoss(weight=w) on the module path"""
    from mnasnet_pytorch_amd import DistillCrossEntropyLoss
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = torch.tensor([1, 2, 5, 7]).cuda()
    w = _weight()
    res = []
    for crit, native in ((DistillCrossEntropyLoss(alpha=0.0, weight=w), True), (torch.nn.CrossEntropyLoss(weight=w.cuda()), False)):
        tr = Trainer(_model(), lr=1e-3, criterion=crit)
        assert (tr._native_head() is not None) == native
        res.append(([float(tr.step(x, t))], tr.flat_p.clone()))
    print("losses native %r module %r relerr(params) %.3e" % (res[0][0], res[1][0], relerr(res[0][1].cpu(), res[1][1].cpu())))
    assert np.allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert relerr(res[0][1].cpu(), res[1][1].cpu()) < 1e-5
