"""-m gpu: gradient clipping and the weight EMA under the REAL data-parallel step, world_size 2 on ONE MI355X (the set-up of
tests/test_gpu_world2.py: two fresh child processes on cuda:0, Trainer(distributed=True), gloo on device tensors).

The norm is taken after the all-reduce with grad_scale = 1/2 -- the norm of the mean gradient -- by a deterministic kernel, so both
ranks derive the same bits for the norm, the coefficient and hence the update and the shadow, with no collective more:
  * flat_p, flat_ema and the three steps' last_norm are BIT-equal on both ranks after three clipped SGD steps;
  * they equal the one-process emulation (two forward+backward passes accumulated into one gradient buffer, grad_scale 0.5) within
    the bounds tests/test_gpu_world2.py states for SGD: the summed gradient of step 1 to 1e-6 relative L2 (the two sums differ in
    association only), hence the norm of step 1 to 1e-6 + 2 * 2^-24 relative; the three-step update to 1e-2 relative L2 and 5e-6
    per element.  Those bounds were stated for the unclipped step at the same learning rate; a coefficient < 1 shrinks every
    update and its divergence with it, and the coefficients' own difference (the norms', 1.2e-6 relative) is far inside.  The
    shadow is a convex combination of the parameters of steps 0..3, so the per-element bound holds for it too."""
import os
import subprocess
import sys

import pytest
import torch

import cases as C  # noqa: F401  (sys.path set-up shared with the worker)
from gradclip_world2_worker import LR
from test_gpu_train import _no_dropout, build
from test_gpu_world2 import GPU_PROCESS_LIMIT, _free_port
from world2_worker import rank_batch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CLIP, DECAY = 1.0, 0.9


def _run(tmp_path, world=2):
    assert world + 1 <= GPU_PROCESS_LIMIT
    port = _free_port()
    outs = [str(tmp_path / ("rank%d.pt" % r)) for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "gradclip_world2_worker.py"), str(r), str(world), str(port), outs[r],
                               repr(CLIP), repr(DECAY)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace")[-3000:])
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, logs[r])
    return [torch.load(o) for o in outs]


def _emulate():
    from mnasnet_pytorch_amd.train_step import Trainer
    m = build("512", proj_gamma=0.1).train()
    _no_dropout(m)
    tr = Trainer(m, lr=LR, optimizer="sgd", clip_grad_norm=CLIP, ema_decay=DECAY)
    tr.optimizer.grad_scale = 0.5
    batches = [tuple(v.cuda() for v in rank_batch(r)) for r in range(2)]
    p0 = tr.flat_p.detach().cpu().clone()
    norms, g1 = [], None
    for step in range(3):
        tr.optimizer.zero_grad()
        for x, t in batches:
            tr.forward_backward(x, t)
        if step == 0:
            g1 = tr.flat_g.detach().cpu().clone()
        tr.optimizer.step()
        norms.append(tr.last_grad_norm.clone())
    return {"flat_p": tr.flat_p.detach().cpu(), "flat_ema": tr.flat_ema.detach().cpu(), "flat_p0": p0, "flat_g1": g1,
            "norms": torch.cat(norms).cpu(), "stats": tuple(tr.grad_stats())}


def test_clip_and_ema_world2_one_gpu(tmp_path):
    r0, r1 = _run(tmp_path)
    assert r0["world"] == r1["world"] == 2
    print("world-2 clip: norms %s stats %s" % (r0["norms"].tolist(), r0["stats"]))
    # one model, one shadow, one norm on both ranks, bit for bit
    assert torch.equal(r0["flat_p0"], r1["flat_p0"]) and torch.equal(r0["flat_ema0"], r0["flat_p0"])
    for k in ("flat_p", "flat_ema", "norms", "flat_g1", "flat_ema0"):
        assert torch.equal(r0[k], r1[k]), k
    assert r0["stats"] == r1["stats"]
    assert bool(torch.isfinite(r0["flat_p"]).all()) and bool(torch.isfinite(r0["flat_ema"]).all())
    assert r0["stats"][2:] == (3, 3, 0)                      # steps, clipped_steps, skipped_steps: every step clipped
    assert bool((r0["norms"] > CLIP).all())
    assert not torch.equal(r0["flat_p"], r0["flat_p0"]) and not torch.equal(r0["flat_ema"], r0["flat_p"])
    # ... and the one-process emulation
    emu = _emulate()
    assert torch.equal(emu["flat_p0"], r0["flat_p0"]) and emu["stats"][2:] == (3, 3, 0)
    eg = float((r0["flat_g1"].double() - emu["flat_g1"].double()).norm() / emu["flat_g1"].double().norm())
    en = abs(float(r0["norms"][0]) - float(emu["norms"][0])) / float(emu["norms"][0])
    upd = (emu["flat_p"] - emu["flat_p0"]).double()
    eu = float(((r0["flat_p"] - r0["flat_p0"]).double() - upd).norm() / upd.norm())
    d3 = float((r0["flat_p"] - emu["flat_p"]).abs().max())
    de = float((r0["flat_ema"] - emu["flat_ema"]).abs().max())
    print("world-2 clip vs emulation: gradient of step 1 rel-L2 %.3e, its norm rel %.3e; 3-step update rel-L2 %.3e, max |diff| p %.3e "
          "ema %.3e" % (eg, en, eu, d3, de))
    assert eg < 1e-6 and en <= 1e-6 + 2.0 ** -23
    assert eu < 1e-2 and d3 < 5e-6 and de < 5e-6
