"""-m gpu: the multi-label Trainer.validate on a world of 2 on ONE MI355X (two fresh child processes on cuda:0 over gloo, in the
manner of tests/test_gpu_metrics_world2.py).  Each rank validates a different half of the set; after the meters' all_reduce both
ranks hold identical blocks whose integer fields are those of a single-process pass over the WHOLE set, and whose double sums are the
sums of the halves exactly (the whole within 4 * 2^-52 relative: the same terms added in another order)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

import cases as C  # noqa: F401  (sys.path set-up shared with the worker)
from multilabel_world2_worker import INT_FIELDS, SUM_FIELDS, build_trainer, record, val_set

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_multilabel_validate_world2_one_gpu(tmp_path):
    world = 2                                            # 2 extra processes with the GPU open, next to this one
    port = _free_port()
    outs = [str(tmp_path / ("rank%d.pt" % r)) for r in range(world)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "multilabel_world2_worker.py"), str(r), str(world), str(port), outs[r]],
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
    m, tr = build_trainer()
    whole = record(tr.validate([(x.cuda(), t.cuda()) for x, t in val_set()]))
    halves = [record(tr.validate([(x.cuda(), t.cuda()) for i, (x, t) in enumerate(val_set()) if i % 2 == r])) for r in range(2)]
    print("single process:", whole, "\nrank 0:", r0["reduced"], "\nrank 1:", r1["reduced"])
    assert r0["world"] == r1["world"] == 2 and r0["training"] and r1["training"]
    assert torch.equal(r0["block"], r1["block"]) and r0["reduced"] == r1["reduced"]      # identical blocks on both ranks
    red = r0["reduced"]
    for k in INT_FIELDS:
        assert red[k] == whole[k], k                                       # the counts of the whole set, exactly
    assert (red["samples"], red["steps"], red["f1_n"]) == (32, 4, 12)
    # last update over ranks = the sum of the two ranks' last batches
    assert red["last_n"] == 16 and red["last"] == tuple(a + b for a, b in zip(halves[0]["last"], halves[1]["last"]))
    assert red["last_sums"] == tuple(a + b for a, b in zip(halves[0]["last_sums"], halves[1]["last_sums"]))
    for i, n in enumerate((16, 16, 6)):
        assert red["val"][i] == red["last_sums"][i] / n                    # val over the global last batch: the weighted mean
    # the double sums: the same four terms, added as (a + c) + (b + d) instead of ((a + b) + c) + d
    for i, k in enumerate(SUM_FIELDS):
        assert red[k] == halves[0][k] + halves[1][k], k
        assert abs(red[k] - whole[k]) <= 4 * 2.0 ** -52 * abs(whole[k]), k
        assert abs(red["avg"][i] - whole["avg"][i]) <= 4 * 2.0 ** -52 * abs(whole["avg"][i]), k
    # rank 1 alone, before the buffer broadcast, saw another model: the broadcast is what made it agree
    assert r0["local_before_sync"] == halves[0]
    assert r1["local_before_sync"]["loss_sum"] != halves[1]["loss_sum"]
