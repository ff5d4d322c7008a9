"""CPU (no GPU needed): the frozen stage prefix.

* launch_plan.LaunchPlan(first_trainable=b): the backward ends at step b.  For every stage boundary the forward list is the full
  program's, the segments behind the boundary stage are the full program's line for line (make_launch_plan_golden.dump_program), the
  frozen stages get no segment, no gradient pointer outside the trainable ranges and no buffer.
* Engine.first_trainable_step() over requires_grad patterns; FineTuneModelPool.freeze(upto=k).
* train_step.BucketSchedule.begin_step(first_trainable_stage=k) on gloo, world 2: the frozen tail of the flat gradient buffer is left
  out of the all-reduce."""
import contextlib
import io
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import make_launch_plan_golden as G
from mnasnet_pytorch_amd import FineTuneModelPool, Mnasnet
from mnasnet_pytorch_amd.engine import Engine
from test_ddp_gloo import _free_port, _stub_layout

SHAPES = [(256, 224, 224), (3, 64, 96)]
_FLAT = re.compile(r"flat_grad(?:\+(\d+))?")


def _stage_first(eng):
    """first step of every stage; stage 8 (one past the last) = len(steps)"""
    first = {}
    for i, (_, _, st) in enumerate(eng.steps):
        first.setdefault(st, i)
    first[max(first) + 1] = len(eng.steps)
    return first


def _split(lines):
    """(header, forward lines, {stage: backward lines})"""
    head = [ln for ln in lines if not ln.startswith(("fwd ", "bwd"))]
    fwd = [ln for ln in lines if ln.startswith("fwd ")]
    bwd = {}
    for ln in lines:
        if ln.startswith("bwd"):
            bwd.setdefault(int(ln.split(" ", 1)[0][3:]), []).append(ln)
    return head, fwd, bwd


def _grad_elems(lines):
    """element offsets into flat_grad named by the ops of `lines`"""
    out = set()
    for ln in lines:
        for m in _FLAT.finditer(ln.split(" p=", 1)[1]):
            off = int(m.group(1) or 0)
            assert off % 4 == 0
            out.add(off // 4)
    return out


def _keep_bytes(prog):
    return sum(t.numel() * t.element_size() for t in prog.keep)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("se", [0.0, 0.25], ids=["se0", "se1"])
@pytest.mark.parametrize("ccf", [False, True], ids=["ccf0", "ccf1"])
def test_truncated_plans(ccf, se, shape):
    N, H, W = shape
    cfg = dict(ccf=ccf, se=se, shape=shape, training=True)
    eng, full, model = G.build_program(cfg)             # program() called without the keyword
    full_lines = G.dump_program(eng, full)
    _, full_fwd, full_bwd = _split(full_lines)
    full_bytes = _keep_bytes(full)
    assert full.first_trainable == 0 and sorted(full_bwd, reverse=True) == list(range(7, -1, -1))
    first = _stage_first(eng)
    assert sorted(first) == list(range(9))
    del full
    prev_bytes = None
    for k in range(9):
        eng.reset_programs()
        prog = eng.program(N, H, W, True, False, True, False, first_trainable=first[k])
        lines = G.dump_program(eng, prog)
        nbytes = _keep_bytes(prog)
        segs = [st for st, _, _ in prog.bwd_segments]
        assert prog.first_trainable == first[k]
        del prog
        if k == 0:
            assert lines == full_lines
        _, fwd, bwd = _split(lines)
        assert fwd == full_fwd, k
        assert segs == list(range(7, k - 1, -1)) and sorted(bwd, reverse=True) == segs, (k, segs)
        for st in range(k + 1, 8):
            assert bwd[st] == full_bwd[st], (k, st)
        # gradient pointers: none outside the ranges of the stages >= k, none of the full plan's for those stages lost
        ranges = [tuple(eng.stage_ranges[s]) for s in eng.stage_ranges if s >= k]
        got = _grad_elems([ln for st in segs for ln in bwd[st]])
        assert all(any(a <= e < b for a, b in ranges) for e in got), k
        assert got == _grad_elems([ln for st in range(k, 8) for ln in full_bwd[st]]), k
        # buffers
        assert nbytes <= (full_bytes if prev_bytes is None else prev_bytes), (k, nbytes, prev_bytes)
        if k >= 2:
            assert nbytes < full_bytes, (k, nbytes, full_bytes)
        prev_bytes = nbytes
    del model


def test_first_trainable_is_part_of_the_program_key_and_checked():
    eng, full, model = G.build_program(dict(ccf=False, shape=(2, 32, 32), training=True))
    a = eng.program(2, 32, 32, True, False, True, False, first_trainable=3)
    assert a is not full and a.first_trainable == 3
    assert eng.program(2, 32, 32, True, False, True, False, first_trainable=3) is a
    assert eng.program(2, 32, 32, True, False, True, False) is full
    assert len(eng.programs) == 2 and all(len(key) == 9 for key in eng.programs)
    none = eng.program(2, 32, 32, True, False, True, False, first_trainable=len(eng.steps))
    assert none.bwd_segments == [] and none.patch_gout is None
    with pytest.raises(RuntimeError, match="no backward"):
        none.run_backward(torch.zeros(2, 320))
    for bad in (-1, len(eng.steps) + 1):
        with pytest.raises(ValueError):
            eng.program(2, 32, 32, True, False, True, False, first_trainable=bad)
    with pytest.raises(ValueError):
        eng.program(2, 32, 32, True, True, True, False, first_trainable=3)       # an input gradient needs the whole backward
    with pytest.raises(ValueError):
        eng.program(2, 32, 32, False, False, True, False, first_trainable=3)      # inference has none
    del model


def test_frozen_statistics_program_is_truncated_the_same_way():
    m = Mnasnet(cut_channels_first=False)
    m.train()
    m.features.eval()
    eng = Engine(m.features)
    eng.ensure_setup(torch.device("cpu"))
    first = _stage_first(eng)
    full = G.dump_program(eng, eng.program(3, 64, 96, True, False, True, False, frozen_bn=True))
    _, full_fwd, full_bwd = _split(full)
    for k in (1, 3, 6):
        eng.reset_programs()
        prog = eng.program(3, 64, 96, True, False, True, False, frozen_bn=True, first_trainable=first[k])
        _, fwd, bwd = _split(G.dump_program(eng, prog))
        assert fwd == full_fwd and sorted(bwd, reverse=True) == list(range(7, k - 1, -1))
        assert all(bwd[st] == full_bwd[st] for st in range(k + 1, 8))
        assert any(" BWD_POST_FROZEN " in ln for ln in bwd[k])


# ---- boundary detection ---------------------------------------------------------------------------------------------------------
def _pool(ccf=False, **kw):
    return FineTuneModelPool(Mnasnet(cut_channels_first=ccf, **kw), "mnasnet", 10, "512")


@pytest.mark.parametrize("kw", [dict(), dict(ccf=True), dict(se_ratio=0.25)], ids=["ccf0", "ccf1", "se"])
def test_first_trainable_step(kw):
    m = _pool(**kw)
    eng = m.features._engine()
    first = _stage_first(eng)
    nsteps = len(eng.steps)
    assert eng.first_trainable_step() == 0
    for k in range(9):
        m.freeze(upto=k)
        assert eng.first_trainable_step() == first[k], k
        assert eng.step_stage(eng.first_trainable_step()) == k
    with contextlib.redirect_stdout(io.StringIO()):
        m.freeze()
        assert eng.first_trainable_step() == nsteps
        m.unfreeze()
    assert eng.first_trainable_step() == 0
    # only stage 3 frozen: the stem still trains
    for p in m.features[3].parameters():
        p.requires_grad = False
    assert eng.first_trainable_step() == 0
    # stages 0-2 frozen plus one bn.weight behind the boundary: the boundary does not move
    m.freeze(upto=3)
    bn_w = [p for n, p in m.features[5].named_parameters() if n.endswith("bn.weight")][0]
    bn_w.requires_grad = False
    assert eng.first_trainable_step() == first[3]
    # every parameter a step owns counts: one trainable bn.bias in stage 1 pulls the boundary to that ConvBlock's step
    bn_b = [p for n, p in m.features[1].named_parameters() if n.endswith("bn.bias")][-1]
    bn_b.requires_grad = True
    assert eng.first_trainable_step() == first[1] + 1       # (SepConv's second ConvBlock)
    m.freeze(upto=0)
    assert all(p.requires_grad for p in m.features.parameters())


def test_shared_block_flips_all_its_applications():
    m = _pool()
    eng = m.features._engine()
    first = _stage_first(eng)
    seq = m.features[2].sequence
    blocks = [b for b in seq if type(b).__name__ == "MBConv_block"]
    assert len(blocks) == 3 and blocks[0] is blocks[1] is blocks[2]
    assert [op for op, _, st in eng.steps if st == 2] == ["block", "block", "block", "conv"]
    for p in blocks[0].parameters():
        p.requires_grad = False
    assert eng.first_trainable_step() == 0                   # the stem trains
    m.freeze(upto=2)
    for p in blocks[0].parameters():
        p.requires_grad = False
    assert eng.first_trainable_step() == first[2] + 3        # all three applications are frozen: the stage's stride-2 conv is first
    for p in blocks[0].parameters():
        p.requires_grad = True
    assert eng.first_trainable_step() == first[2]


def test_squeeze_excite_parameters_belong_to_their_block():
    m = _pool(se_ratio=0.25)
    eng = m.features._engine()
    first = _stage_first(eng)
    m.freeze(upto=8)
    se_params = [p for n, p in m.features[4].named_parameters() if ".se." in n]
    assert se_params
    se_params[0].requires_grad = True
    b = eng.first_trainable_step()
    assert first[4] <= b < first[5] and eng.steps[b][0] == "block"
    assert any(p is se_params[0] for p in eng.step_params(b))


# ---- FineTuneModelPool.freeze(upto=) --------------------------------------------------------------------------------------------------
def test_freeze_upto_surface():
    m = _pool()
    n = len(m.features)
    assert n == 8
    for bad in (-1, n + 1, 2.0, "3", True):
        with pytest.raises(ValueError):
            m.freeze(upto=bad)
    assert all(p.requires_grad for p in m.parameters())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        for k in (5, 2, 7, 0, n):
            m.freeze(upto=k)
            for i, child in enumerate(m.features):
                assert all(p.requires_grad == (i >= k) for p in child.parameters()), (k, i)
            assert all(p.requires_grad for p in m.classifier.parameters())
    assert buf.getvalue() == ""
    with contextlib.redirect_stdout(buf):
        m.freeze()
    assert buf.getvalue() == "Features frozen\n" and not any(p.requires_grad for p in m.features.parameters())
    assert all(p.requires_grad for p in m.classifier.parameters())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        m.unfreeze()
    assert buf.getvalue() == "Features unfrozen\n" and all(p.requires_grad for p in m.parameters())


def test_freeze_upto_is_independent_of_freeze_bn():
    m = _pool().train()
    m.freeze(upto=4)
    assert all(mod.training for mod in m.features.modules())            # train-mode BatchNorm everywhere, frozen stages included
    m.freeze_bn()
    assert not any(mod.training for mod in m.features.modules()) and m.classifier.training
    assert [all(p.requires_grad for p in c.parameters()) for c in m.features] == [False] * 4 + [True] * 4
    m.freeze(upto=2)
    assert m.bn_frozen and not any(mod.training for mod in m.features.modules())
    m.freeze_bn(False)
    assert all(mod.training for mod in m.features.modules())
    assert [all(p.requires_grad for p in c.parameters()) for c in m.features] == [False] * 2 + [True] * 6


# ---- data parallel: the frozen tail stays out of the all-reduce -------------------------------------------------------------------
def _prefix_sched_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    try:
        from mnasnet_pytorch_amd.train_step import BucketSchedule
        n_head, ranges, n_eng = _stub_layout()
        n = n_head + n_eng
        flat = torch.zeros(n)
        sched = BucketSchedule(flat, n_head, ranges, early_bucket_stage=5)
        split = n_head + ranges[5][1]
        oks = {}
        # (boundary stage, expected bounds, expected log): below early_stage, above it, the default call, everything frozen
        cases = [
            (3, [0, split, n_head + ranges[3][1]],
             [("stage", 7), ("stage", 6), ("stage", 5), ("launch", 0), ("stage", 4), ("stage", 3), ("launch", 1)]),
            (6, [0, n_head + ranges[6][1], n_head + ranges[6][1]], [("stage", 7), ("stage", 6), ("launch", 0), ("launch", 1)]),
            (None, [0, split, n], [("stage", 7), ("stage", 6), ("stage", 5), ("launch", 0)] + [("stage", s) for s in (4, 3, 2, 1, 0)] + [("launch", 1)]),
            (8, [0, n_head, n_head], [("launch", 0), ("launch", 1)]),
            (5, [0, split, split], [("stage", 7), ("stage", 6), ("stage", 5), ("launch", 0), ("launch", 1)]),
        ]
        for step, (k, bounds, want_log) in enumerate(cases):
            flat.fill_(-7.0)                     # the sentinel: whatever no collective touches keeps it
            if k is None:
                sched.begin_step()
            else:
                sched.begin_step(first_trainable_stage=k)
            kk = 0 if k is None else k
            flat[:n_head] = 1.0 + rank
            for st in sorted(ranges, reverse=True):
                if st < kk:
                    continue                     # the engine's backward has no segment for a stage in front of the boundary
                a, b = ranges[st]
                flat[n_head + a:n_head + b] = (st + 1) * (1.0 + rank) + step
                sched.on_stage_done(st)
            sched.finish()
            tot = sum(1.0 + r for r in range(world))
            exp = torch.full((n,), -7.0)
            exp[:n_head] = tot
            for st in ranges:
                if st >= kk:
                    a, b = ranges[st]
                    exp[n_head + a:n_head + b] = (st + 1) * tot + step * world
            oks[(k, "bounds")] = sched.buckets.bounds == bounds
            oks[(k, "log")] = sched.log == want_log
            oks[(k, "sum over ranks, frozen tail untouched")] = bool(torch.equal(flat, exp))
            oks[(k, "handles drained")] = sched.buckets.handles == []
        q.put((rank, oks))
    finally:
        dist.destroy_process_group()


def test_bucket_schedule_leaves_the_frozen_prefix_out_world2_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_prefix_sched_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, oks in res:
        assert all(oks.values()), (rank, [k for k, v in oks.items() if not v])
