"""-m gpu: parameter groups, AdamW and LAMB through the Trainer, on the smallest setup of test_trainer_end_to_end (4 x 3 x 64 x 64,
head '512', dropout off, three steps)."""
import numpy as np
import pytest
import torch

import cases as C
from test_gpu_train import _no_dropout, build, rl2

pytestmark = pytest.mark.gpu

WD = 1e-2


def _batch():
    return C.det_input((4, 3, 64, 64)).cuda(), torch.tensor([1, 3, 5, 7]).cuda()


def _model():
    m = build("512", 10, proj_gamma=0.1).train()
    _no_dropout(m)
    return m


def test_adamw_with_norm_bias_groups_matches_torch():
    """Trainer(param_groups=norm_bias_groups, decoupled_weight_decay=True) against the same model stepped through the module path
    with torch.optim.AdamW over the same two groups: the losses within test_trainer_matches_torch_optimizer_path's tolerances for
    Adam (5e-3 of the first, 3e-2 of the third), the parameters within the looser of the two.  This is a test of the PLUMBING --
    the helper's groups reach the optimizer, the flags are set, every step is one _seg call, training proceeds as torch's does: a
    3e-2 bound on the parameters is about the size of three Adam steps and cannot tell AdamW from Adam.  The arithmetic of the
    grouped and decoupled updates is held by test_gpu_param_groups.py (bit for bit against the plain kernels, 1e-6 against
    torch.optim.AdamW, per-element brackets).  The relative difference of the UPDATES p - p0 is printed, not asserted: the two
    sides' gradients differ by the bf16 roundings of two forward / backward paths, which Adam's normalisation turns into
    differences of the size of the step wherever a gradient is small."""
    from mnasnet_pytorch_amd.train_step import Trainer, norm_bias_groups
    x, t = _batch()
    m1 = _model()
    start = torch.cat([p.detach().flatten().cpu().clone() for _, p in m1.named_parameters()])
    opt = torch.optim.AdamW(norm_bias_groups(m1, WD), lr=1e-3)
    assert [g["weight_decay"] for g in opt.param_groups] == [WD, 0.0]
    crit = torch.nn.CrossEntropyLoss()
    l1 = []
    for _ in range(3):
        loss = crit(m1(x), t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        l1.append(float(loss.detach()))
    m2 = _model()
    tr = Trainer(m2, lr=1e-3, param_groups=lambda m: norm_bias_groups(m, WD), decoupled_weight_decay=True)
    groups = tr.optimizer.param_groups
    assert len(groups) == 2 and [(g["weight_decay"], g["decoupled"]) for g in groups] == [(WD, True), (0.0, True)]
    assert all(p.ndim <= 1 for p in groups[1]["params"]) and len(groups[1]["params"]) == 81 + 2
    l2 = [float(tr.step(x, t)) for _ in range(3)]
    assert tr.optimizer.seg_calls == 3
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    names = [k for k, _ in m1.named_parameters()]
    err = rl2(torch.cat([sd2[k].flatten().cpu() for k in names]), torch.cat([sd1[k].flatten().cpu() for k in names]))
    u1 = torch.cat([sd1[k].flatten().cpu() for k in names]) - start
    u2 = torch.cat([sd2[k].flatten().cpu() for k in names]) - start
    assert float(u1.norm()) > 0 and float(u2.norm()) > 0
    print("adamw: losses torch", l1, "trainer", l2, "parameters rl2 %.3g, updates rl2 %.3g" % (err, rl2(u2, u1)))
    assert abs(l1[0] - l2[0]) <= 5e-3 * abs(l1[0]), (l1, l2)
    assert abs(l1[2] - l2[2]) <= 3e-2 * abs(l1[2]), (l1, l2)
    assert err <= 3e-2


def test_lamb_trainer_with_clipping_ema_and_freeze():
    """optimizer='lamb' with norm_bias_groups, clipping and the EMA: finite losses, trust_ratios() named and finite, the no-decay
    group's ratios exactly 1; after freeze(upto=4) the frozen stages' parameters stay bitwise as they were and a step is still one
    _seg call."""
    from mnasnet_pytorch_amd.train_step import Trainer, norm_bias_groups
    x, t = _batch()
    m = _model()
    tr = Trainer(m, lr=1e-3, optimizer="lamb", param_groups=lambda mod: norm_bias_groups(mod, WD), clip_grad_norm=1.0, ema_decay=0.9)
    assert tr.optimizer.trust_ratio == "lamb" and type(tr.optimizer).__name__ == "FlatAdam"
    losses = [float(tr.step(x, t)) for _ in range(3)]
    ratios = tr.trust_ratios()
    names = dict(m.named_parameters())
    st = tr.grad_stats()
    print("lamb: losses", losses, st, "ratios of %d tensors in [%.3g, %.3g]" % (len(ratios), min(ratios.values()), max(ratios.values())))
    assert np.isfinite(losses).all() and st.steps == 3 and tr.optimizer.seg_calls == 3
    assert set(ratios) == set(names) and np.isfinite(list(ratios.values())).all()
    assert all(ratios[k] == 1.0 for k, p in names.items() if p.ndim <= 1)
    assert any(ratios[k] != 1.0 for k, p in names.items() if p.ndim > 1)
    assert not torch.equal(tr.flat_ema, tr.flat_p)
    # gradual unfreezing: features[:4] frozen
    m.freeze(upto=4)
    frozen = {k: p.detach().clone() for k, p in names.items() if not p.requires_grad}
    assert frozen and all(k.startswith("features.") and int(k.split(".")[1]) < 4 for k in frozen)
    calls = tr.optimizer.seg_calls
    loss = float(tr.step(x, t))
    assert np.isfinite(loss) and tr.optimizer.seg_calls == calls + 1
    for k, v in frozen.items():
        assert torch.equal(names[k].detach(), v), k
    after = tr.trust_ratios()
    assert set(after) == set(names) - set(frozen)
    # "lars" is SGD with the LARS ratio
    tr2 = Trainer(_model(), lr=1e-2, optimizer="lars", momentum=0.9, weight_decay=1e-4)
    assert tr2.optimizer.trust_ratio == "lars" and type(tr2.optimizer).__name__ == "FlatSGD"
    assert np.isfinite(float(tr2.step(x, t))) and tr2.optimizer.seg_calls == 1 and len(tr2.trust_ratios()) == len(names)


def test_trainer_without_the_new_options_steps_as_before():
    """A trainer built without any of the new options never takes the _seg path: its optimizer step is, bit for bit, a FlatAdam
    driven through _launch directly (the parent commit's step: one mnas_adam_step per trainable run) on the same gradients."""
    from mnasnet_pytorch_amd.train_step import FlatAdam, Trainer
    x, t = _batch()
    tr = Trainer(_model(), lr=1e-3, weight_decay=1e-2)
    n = tr.flat_p.numel()
    flat_p, flat_g = tr.flat_p.clone(), torch.zeros(n, device="cuda")
    par = torch.nn.Parameter(flat_p.view(n))
    par.data = flat_p.view(n)
    twin = FlatAdam([par], flat_p, flat_g, lr=1e-3, weight_decay=1e-2)
    for _ in range(3):
        tr.optimizer.zero_grad()
        tr.forward_backward(x, t)
        flat_g.copy_(tr.flat_g)
        tr.optimizer.step()
        twin.step_count += 1
        for a, b in twin._trainable_runs():
            twin._launch(a, b, twin.param_groups[0])
        assert torch.equal(flat_p, tr.flat_p) and torch.equal(twin.flat_m, tr.flat_m) and torch.equal(twin.flat_v, tr.flat_v)
    assert tr.optimizer.seg_calls == 0 and not tr.optimizer._grouped() and len(tr.optimizer.param_groups) == 1
    assert tr.optimizer.trust_ratios() == {} and tr.trust_ratios() == {}


def test_one_dict_group_in_torch_order_with_a_frozen_prefix():
    """The idiomatic torch form, ONE group dict holding model.parameters() (features first; the flat buffer holds the head first),
    then freeze(upto=4): the plain launches must run over the trainable tensors' own ranges -- the frozen stages bitwise unchanged,
    the head and the trainable stages moving -- over the runs a trainer built without param_groups takes."""
    from mnasnet_pytorch_amd.train_step import Trainer
    x, t = _batch()
    m, ref = _model(), _model()
    tr = Trainer(m, lr=1e-3, weight_decay=1e-2, param_groups=[{"params": list(m.parameters())}])
    tr_ref = Trainer(ref, lr=1e-3, weight_decay=1e-2)             # (for its runs only: it is not stepped)
    assert len(tr.optimizer.param_groups) == 1 and not tr.optimizer._grouped()
    assert [id(p) for p in tr.optimizer.param_groups[0]["params"]] != [id(p) for p in tr.optimizer._all_params]
    for mod in (m, ref):
        mod.freeze(upto=4)
    assert tr.optimizer._trainable_runs() == tr_ref.optimizer._trainable_runs()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    losses = [float(tr.step(x, t)) for _ in range(2)]
    assert np.isfinite(losses).all() and tr.optimizer.seg_calls == 0
    moved = {k: not torch.equal(p.detach(), before[k]) for k, p in m.named_parameters()}
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert not moved[k], k                                # a frozen stage: neither Adam nor the decay touched it
        elif k.startswith("classifier.") or p.ndim > 1:
            assert moved[k], k                                    # the head and every trainable weight train
    assert sum(not p.requires_grad for p in m.parameters()) > 0
