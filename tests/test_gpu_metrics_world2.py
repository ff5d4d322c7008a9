"""-m gpu: Trainer.validate on a world of 2 on ONE MI355X (two fresh child processes on cuda:0 over gloo, in the manner of
tests/test_gpu_world2.py).  Each rank validates a different half of the set; after the meters' all_reduce both ranks hold the counts
of the WHOLE set, equal to a single-process pass over it.  Rank 1 starts from other parameters and other BatchNorm statistics: the
halves only add up to the single-process result because Trainer broadcasts rank 0's parameters and validate() its buffers."""
import os
import socket
import subprocess
import sys

import pytest
import torch

import cases as C  # noqa: F401  (sys.path set-up shared with the worker)
from metrics_world2_worker import build_model, record, val_set

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_validate_world2_one_gpu(tmp_path):
    world = 2                                            # 2 extra processes with the GPU open, next to this one
    port = _free_port()
    outs = [str(tmp_path / ("rank%d.pt" % r)) for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "metrics_world2_worker.py"), str(r), str(world), str(port), outs[r]],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
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
    r0, r1 = (torch.load(o) for o in outs)
    # single process, the whole set, rank 0's model
    from mnasnet_pytorch_amd.train_step import Trainer
    m = build_model()
    tr = Trainer(m, lr=1e-3)
    whole = record(tr.validate([(x.cuda(), t.cuda()) for x, t in val_set()]))
    halves = [record(tr.validate([(x.cuda(), t.cuda()) for i, (x, t) in enumerate(val_set()) if i % 2 == r])) for r in range(2)]
    print("single process:", whole, "\nrank 0:", r0["reduced"], "\nrank 1:", r1["reduced"])
    assert r0["world"] == r1["world"] == 2 and r0["training"] and r1["training"]
    assert r0["reduced"] == r1["reduced"]                                  # one result on both ranks, bit for bit
    red = r0["reduced"]
    for k in ("steps", "samples", "loss_samples", "correct", "nonfinite_steps"):
        assert red[k] == whole[k], k                                       # the counts of the whole set, exactly
    assert red["samples"] == 32 and red["steps"] == 4
    # last update over ranks = the sum of the two ranks' last batches
    assert red["last_n"] == 16 and red["last_correct"] == {k: halves[0]["last_correct"][k] + halves[1]["last_correct"][k] for k in (1, 5)}
    # the loss: the same four fp32 losses times 8, summed in double as (a + c) + (b + d) instead of ((a + b) + c) + d
    assert red["loss_sum"] == halves[0]["loss_sum"] + halves[1]["loss_sum"]
    assert abs(red["loss_sum"] - whole["loss_sum"]) <= 4 * 2.0 ** -52 * abs(whole["loss_sum"])
    assert abs(red["loss_avg"] - whole["loss_avg"]) <= 4 * 2.0 ** -52 * abs(whole["loss_avg"])
    # rank 1 alone, before the buffer broadcast, saw another model (its statistics were scaled): the broadcast is what made it agree
    assert r0["local_before_sync"] == halves[0]
    assert r1["local_before_sync"]["loss_sum"] != halves[1]["loss_sum"]
    assert torch.equal(r0["rm0"], r1["rm0"]) and torch.equal(r0["rm0"], m.features[0].bn.running_mean.detach().cpu())
