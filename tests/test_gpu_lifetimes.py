"""-m gpu: the autograd contract of the engine (mnasnet_pytorch_amd/engine.py Engine / Program / _Lease) and of the native head
(head.py _HeadFn) when more than one forward is alive, when other forwards run between a forward and its backward, when the launch
lists replay as hipGraphs through the module path, and when state a backward reads has changed since its forward.

No kernel is held to a bound here (tests/test_gpu_kernels.py ... do that): every comparison is between two schedules of the SAME
launches on the SAME numbers, so the tolerance is equality of bits.  Why equality is the right bound: a Program owns its
activations and BatchNorm coefficient blocks, a train-mode backward reads nothing else that differs between two programs of one
model with fixed weights (the packed weights are re-packed from the same values by every forward), and the accumulate kernels
compute grad = grad + (completed sum) (csrc/mnas_elementwise.hip `*d = (accumulate ? *d : 0.f) + s`, bn_bwd_finalize_body), so the
final ``.grad`` depends on the ORDER of the backwards and on nothing else.  The reference of an overlapped schedule is therefore the
serial schedule (forward, backward, next job, no zero_grad) with the same backward order -- not g1 + g2, which rounds differently
for a list-multiplied block: ((0 + a1) + a2) + b1 ... -- and, for the running statistics, the serial schedule in forward order.

Models: FineTuneModelPool (head "512", 10 classes, proj_gamma 0.1: stem, shared blocks, head) at (2,3,64,64) / (3,3,64,96), and one
MBConv_block(16, 3, 3) at (2,16,14,14) / (3,16,14,20), where every parameter has one application."""
import re
from collections import namedtuple
from functools import lru_cache

import pytest
import torch

import cases as C
from gpu_util import bits_equal
from test_gpu_model import fill
from test_gpu_train import _no_dropout, build

pytestmark = pytest.mark.gpu

SHAPES = {"pool": ((2, 3, 64, 64), (3, 3, 64, 96)), "block": ((2, 16, 14, 14), (3, 16, 14, 20))}
KINDS = ("pool", "block")

# mode: "train" (batch statistics) or "frozen" (tracked forward on the running statistics); rg: the input asks for its gradient
Job = namedtuple("Job", "shape seed mode rg")
Result = namedtuple("Result", "outs dx grads stats extra")


def J(shape, seed, mode="train", rg=False):
    return Job(tuple(shape), seed, mode, rg)


@lru_cache(maxsize=None)
def _input(shape, seed):
    """device input of a job; shared, never written (the disturbance tests work on clones)"""
    return C.det_input(shape, seed).cuda()


@lru_cache(maxsize=None)
def _cot(shape, seed):
    return C.cotangent(shape, C.COT_SEED + seed).cuda()


def make(kind, side=False, dropout=False):
    """(model, its engine).  use_side_stream is set before the first forward: it is compiled into the launch lists."""
    if kind == "pool":
        m = build("512", 10, proj_gamma=0.1).train()
        if not dropout:
            _no_dropout(m)
        eng = m.features._engine()
    else:
        from mnasnet_pytorch_amd import MBConv_block
        m = MBConv_block(16, 3, 3)
        fill(m, "block_16_3_3")
        m = m.cuda().train()
        eng = m._engine()
    eng.use_side_stream = side
    return m, eng


def set_mode(kind, m, mode):
    m.train(mode != "eval")
    if mode == "frozen":
        (m.features if kind == "pool" else m).eval()


def snapshot(m):
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}
    stats = {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches_tracked" in k}
    return grads, stats


class Run:
    """One model and the forwards alive on it.  Backwards are separate .backward() calls: their order is the schedule's."""

    def __init__(self, kind, side=False, dropout=False):
        self.kind = kind
        self.m, self.eng = make(kind, side, dropout)
        self.live, self.outs, self.dx, self.extra = {}, {}, {}, []

    def f(self, i, job):
        set_mode(self.kind, self.m, job.mode)
        x = _input(job.shape, job.seed)
        if job.rg:
            x = x.clone().requires_grad_(True)
        out = self.m(x)
        self.live[i] = (x, out, job)
        self.outs[i] = out.detach().clone()

    def b(self, i):
        x, out, job = self.live.pop(i)
        (out * _cot(tuple(out.shape), job.seed)).sum().backward()
        if job.rg:
            self.dx[i] = x.grad.detach().clone()

    def drop(self, i):
        del self.live[i]
        del self.outs[i]

    def nograd(self, shape, seed, mode):
        set_mode(self.kind, self.m, mode)
        with torch.no_grad():
            self.extra.append(self.m(_input(tuple(shape), seed)).clone())

    def programs(self):
        return [p for lst in self.eng.programs.values() for p in lst]

    def result(self):
        assert not self.live
        torch.cuda.synchronize()
        assert not any(p.busy for p in self.programs())
        return Result(self.outs, self.dx, *snapshot(self.m), self.extra)


def play(kind, jobs, sched, side=False):
    """sched: ("f", i) forward of jobs[i] / ("b", i) its backward / ("drop", i) its graph dropped without a backward /
    ("ng", shape, seed, mode) a no-grad forward / ("mode", mode)"""
    r = Run(kind, side)
    for op in sched:
        if op[0] == "f":
            r.f(op[1], jobs[op[1]])
        elif op[0] == "b":
            r.b(op[1])
        elif op[0] == "drop":
            r.drop(op[1])
        elif op[0] == "ng":
            r.nograd(*op[1:])
        else:
            set_mode(kind, r.m, op[1])
    return r.result(), r


_SERIAL = {}


def serial(kind, jobs, order, side=False):
    """the serial schedule: each job's forward, then its backward, in `order`; computed once per (model, jobs, order) and shared"""
    key = (kind, tuple(jobs), tuple(order), side)
    if key not in _SERIAL:
        _SERIAL[key] = play(kind, jobs, [s for i in order for s in (("f", i), ("b", i))], side)[0]
    return _SERIAL[key]


def same_tensor(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
    elif a.element_size() in (2, 4):
        bits_equal(a, b, what)
    else:
        assert torch.equal(a, b), what          # num_batches_tracked (int64)


def same(res, ref, fields, what):
    for f in fields:
        a, b = getattr(res, f), getattr(ref, f)
        if f == "extra":
            assert len(a) == len(b), what
            a, b = dict(enumerate(a)), dict(enumerate(b))
        assert sorted(a) == sorted(b), (what, f)
        assert f == "dx" or len(a) > 0, (what, f)
        for k in a:
            same_tensor(a[k], b[k], "%s: %s[%s]" % (what, f, k))


def overlapped_equals_serial(kind, jobs, fwd, bwd, side=False, inner=()):
    """forwards in `fwd` order (with `inner` ops after them), then backwards in `bwd` order, against the serial runs"""
    sched = [("f", i) for i in fwd] + list(inner) + [("b", i) for i in bwd]
    res, run = play(kind, jobs, sched, side)
    g_ref = serial(kind, jobs, bwd, side)
    same(res, g_ref, ("outs", "dx", "grads"), "%s overlapped vs serial in backward order" % kind)
    same(res, serial(kind, jobs, fwd, side), ("outs", "dx", "stats"), "%s overlapped vs serial in forward order" % kind)
    return res, run


# ---- 1. schedule invariance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [False, True], ids=["main", "side_stream"])
@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["fwd_order", "reverse"])
@pytest.mark.parametrize("kind", KINDS)
def test_two_forwards_of_one_key(kind, order, side):
    """Two inputs of one shape forwarded before either backward: the key's first and second program are both in use.  In the pool
    model this holds the accumulated gradient of the list-multiplied blocks (three / four applications into one slice per backward)
    to the serial run's bits."""
    s0 = SHAPES[kind][0]
    jobs = (J(s0, 7), J(s0, 8))
    res, run = overlapped_equals_serial(kind, jobs, (0, 1), order, side)
    assert max(len(lst) for lst in run.eng.programs.values()) == 2
    assert all(p._built_side == side for p in run.programs())
    assert not bool(torch.equal(res.outs[0], res.outs[1]))
    if kind == "pool":
        shared = [m for op, m, _ in run.eng.steps if op == "block"]
        assert max(sum(1 for m2 in shared if m2[0] is m[0]) for m in shared) == 4        # a block applied four times
        g = res.grads["features.6.sequence.0.sequence.0.conv.weight"]
        assert float(g.abs().max()) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_three_live_forwards_of_two_shapes(kind):
    """Two shapes and batch sizes alive together (two resolution clusters in one step), backward order unlike the forward order:
    gradients against the serial run in backward order, running statistics against the serial run in forward order."""
    s0, s1 = SHAPES[kind]
    jobs = (J(s0, 7), J(s1, 8), J(s0, 9))
    _, run = overlapped_equals_serial(kind, jobs, (0, 1, 2), (2, 0, 1))
    assert sorted(len(lst) for lst in run.eng.programs.values()) == [1, 2]


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["fwd_order", "reverse"])
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_need_dx(kind, order):
    """One input asks for its gradient, the other does not: two program keys of one shape.  The input gradient is compared too."""
    s0 = SHAPES[kind][0]
    jobs = (J(s0, 7, rg=True), J(s0, 8))
    res, run = overlapped_equals_serial(kind, jobs, (0, 1), order)
    assert sorted(res.dx) == [0] and float(res.dx[0].abs().max()) > 0
    assert sorted(len(lst) for lst in run.eng.programs.values()) == [1, 1]


@pytest.mark.parametrize("side", [False, True], ids=["main", "side_stream"])
@pytest.mark.parametrize("kind", KINDS)
def test_eval_forwards_between_forward_and_backward(kind, side):
    """(a) model.eval(), no-grad forwards of the same and of another shape (validation in the middle of a step), model.train(), then
    the backward: the interrupted job's output, gradients and statistics equal the uninterrupted run, and the eval outputs equal
    the same eval forwards after the same train-mode forward with nothing else alive."""
    s0, s1 = SHAPES[kind]
    jobs = (J(s0, 7),)
    evals = [("ng", s0, 8, "eval"), ("ng", s1, 9, "eval")]
    res, _ = play(kind, jobs, [("f", 0)] + evals + [("mode", "train"), ("b", 0)], side)
    same(res, serial(kind, jobs, (0,), side), ("outs", "grads", "stats"), "%s interrupted by eval forwards" % kind)
    alone, _ = play(kind, jobs, [("f", 0), ("drop", 0)] + evals, side)
    same(res, alone, ("extra", "stats"), "%s eval forwards beside a live training forward" % kind)


@pytest.mark.parametrize("kind", KINDS)
def test_recalibration_forward_between_forward_and_backward(kind):
    """(b) a no-grad TRAIN-mode forward (BatchNorm recalibration) between a forward and its backward: it shares the program key
    with the live forward and gets another program; the running statistics advance exactly as forward order says (job, then the
    recalibration batch) and the interrupted job's gradients do not move."""
    s0 = SHAPES[kind][0]
    jobs = (J(s0, 7),)
    recal = ("ng", s0, 8, "train")
    res, _ = play(kind, jobs, [("f", 0), recal, ("b", 0)])
    ref, _ = play(kind, jobs, [("f", 0), ("b", 0), recal])
    same(res, ref, ("outs", "grads", "stats", "extra"), "%s interrupted by a recalibration forward" % kind)
    same(res, serial(kind, jobs, (0,)), ("outs", "grads"), "%s interrupted vs uninterrupted" % kind)
    moved = serial(kind, jobs, (0,)).stats
    assert any(not torch.equal(res.stats[k], moved[k]) for k in moved)


@pytest.mark.parametrize("kind", KINDS)
def test_frozen_statistics_forward_beside_train_forward(kind):
    """(c) a tracked frozen-statistics forward (model.train(); model.features.eval()) alive beside a train-mode one, both
    backwarded: everything equals the serial run, and the running statistics are those of the train-mode job alone."""
    s0 = SHAPES[kind][0]
    jobs = (J(s0, 7), J(s0, 8, "frozen"))
    res, _ = overlapped_equals_serial(kind, jobs, (0, 1), (0, 1))
    same(res, serial(kind, jobs[:1], (0,)), ("stats",), "%s statistics untouched by the frozen job" % kind)
    bias = [k for k in res.grads if k.endswith("conv.bias")]
    assert any(float(res.grads[k].abs().max()) > 0 for k in bias)        # the frozen backward did run (engine.py: s * sum dz)


# ---- 2. hipGraph replay through the module path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_through_module_path(kind):
    """Engine.use_graphs with m(x) -> loss.backward() (not Trainer's static-I/O path): the output and the incoming gradient are
    fresh tensors and two input tensors alternate, so Program._run re-captures the forward list at every call until its four-miss
    limit and then launches it per op (or replays the last capture when the pointers match it).  Eight iterations, gradients
    accumulating: output, every gradient and every statistic after each iteration equal the eager run's.  Linear lists (no side
    stream)."""
    s0 = SHAPES[kind][0]
    xs = (_input(s0, 7), _input(s0, 8))

    def run(graphs):
        m, eng = make(kind)
        eng.use_graphs = graphs
        snaps = []
        for it in range(8):
            out = m(xs[it % 2])
            (out * _cot(tuple(out.shape), 7)).sum().backward()
            snaps.append((out.detach().clone(),) + snapshot(m))
        torch.cuda.synchronize()
        return snaps, eng

    eager, eng0 = run(False)
    graph, eng1 = run(True)
    assert not any(p._graphs for lst in eng0.programs.values() for p in lst)
    for it, ((y0, g0, s0_), (y1, g1, s1_)) in enumerate(zip(eager, graph)):
        same_tensor(y0, y1, "iteration %d output" % it)
        for k in g0:
            same_tensor(g0[k], g1[k], "iteration %d grad %s" % (it, k))
        for k in s0_:
            same_tensor(s0_[k], s1_[k], "iteration %d %s" % (it, k))
    progs = [p for lst in eng1.programs.values() for p in lst]
    assert len(progs) == 1
    p = progs[0]
    assert p._graphs and all(slot["miss"] <= 4 for slot in p._graphs.values())
    # the two inputs are alive together, so the forward list's patched pointer differs from call to call: re-captured, then given up
    assert p._graphs[id(p.fwd_ops)]["miss"] == 4
    assert any(slot["exec"] is not None for slot in p._graphs.values())
    p.destroy_graphs()
    assert all(slot["exec"] is None for slot in p._graphs.values())


# ---- 3. stale state: loud, or the forward-time gradient --------------------------------------------------------------------------
def loud_or_exact(backward, names, exact, what):
    """`backward` must raise a RuntimeError whose message matches `names` (what changed), or `exact` must pass (the gradient of
    the undisturbed run, bit for bit).  A different finite gradient fails in `exact`."""
    try:
        backward()
    except RuntimeError as e:
        assert re.search(names, str(e)), (what, str(e))
        assert "forward again" in str(e), (what, str(e))
        print("%s: raised: %s" % (what, e))
        return "raised"
    exact()
    print("%s: forward-time gradient, bit for bit" % what)
    return "exact"


def _conv_weight(kind, m):
    """a 1x1 conv weight whose packed copies (forward and input-gradient layouts) the backward reads: in the pool model the
    expand conv of stage 3's shared block"""
    return (m.features[3].sequence[0] if kind == "pool" else m).sequence[0].conv.weight


@pytest.mark.parametrize("between", [False, True], ids=["nothing_between", "forward_of_another_shape_between"])
@pytest.mark.parametrize("kind", KINDS)
def test_conv_weight_changed_between_forward_and_backward(kind, between):
    """w.mul_(1.5) between forward A and backward A.  With nothing in between the packed copies still hold the forward's weights;
    with a forward B of another shape in between, B has re-packed the shared buffers from the new weights and A's input-gradient
    kernels would read them against A's activations."""
    s0, s1 = SHAPES[kind]
    jobs = (J(s0, 7, rg=(kind == "block")), J(s1, 8))
    ref = serial(kind, jobs[:1], (0,))
    r = Run(kind)
    r.f(0, jobs[0])
    with torch.no_grad():
        _conv_weight(kind, r.m).mul_(1.5)
    if between:
        r.f(1, jobs[1])
        r.drop(1)
    loud_or_exact(lambda: r.b(0), r"parameter .*conv\.weight.* modified in place",
                  lambda: same(r.result(), ref, ("outs", "dx", "grads"), "weight changed"), "%s conv weight changed" % kind)
    r.live.clear()
    assert not any(p.busy for p in r.programs())


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8_normalised_on_load"])
def test_input_batch_modified_between_forward_and_backward(u8):
    """x.add_(1) between forward and backward: the stem's weight gradient reads the batch in backward -- the caller's own tensor
    for a contiguous fp32 batch (x.float().contiguous() is x) and for a uint8 batch under set_input_normalization."""
    s0 = SHAPES["pool"][0]

    def run(disturb):
        m, eng = make("pool")
        if u8:
            m.normalize_on_device()
            g = torch.Generator().manual_seed(5)
            x = torch.randint(0, 255, s0, generator=g, dtype=torch.uint8).cuda()
        else:
            x = _input(s0, 7).clone()
        out = m(x)
        loss = (out * _cot(tuple(out.shape), 7)).sum()
        if not disturb:
            loss.backward()
            return out.detach().clone(), snapshot(m)[0]
        x.add_(1)
        return loud_or_exact(loss.backward, r"input batch .*modified in place",
                             lambda: [same_tensor(snapshot(m)[0][k], v, k) for k, v in ref.items()], "input batch modified (u8=%s)" % u8)

    _, ref = run(False)
    assert float(ref["features.0.conv.weight"].abs().max()) > 0
    run(True)


def test_head_mode_switched_between_forward_and_backward():
    """model.eval() between forward and backward with the head's dropout on (p = 0.5): the backward belongs to the forward's masks
    (PyTorch keeps the mask of the forward)."""
    s0 = SHAPES["pool"][0]

    def run(disturb):
        torch.manual_seed(0)                      # the head's mask seeds derive from torch.initial_seed() and its call counter
        m, _ = make("pool", dropout=True)
        x = _input(s0, 7).clone().requires_grad_(True)
        out = m(x)
        loss = (out * _cot(tuple(out.shape), 7)).sum()
        if disturb:
            m.eval()
        return m, x, out, loss

    m, x, out0, loss = run(False)
    loss.backward()
    ref, dx0 = snapshot(m)[0], x.grad.clone()
    m, x, out1, loss = run(True)
    bits_equal(out0.detach(), out1.detach(), "the two forwards drew the same masks")

    def exact():
        bits_equal(x.grad, dx0, "input gradient")
        for k, v in snapshot(m)[0].items():
            same_tensor(v, ref[k], k)

    loud_or_exact(loss.backward, r"mode|training|eval", exact, "head: eval() between forward and backward")
    m2, _ = make("pool", dropout=False)
    assert not torch.equal(m2(_input(s0, 7)).detach(), out0.detach())          # dropout was on: the masks mattered


def test_head_weight_changed_between_forward_and_backward():
    """classifier weight changed in place between forward and backward: the head's input gradient would use the new weight."""
    s0 = SHAPES["pool"][0]
    jobs = (J(s0, 7),)
    ref = serial("pool", jobs, (0,))
    r = Run("pool")
    r.f(0, jobs[0])
    with torch.no_grad():
        r.m.classifier[1].weight.mul_(1.5)
    loud_or_exact(lambda: r.b(0), r"classifier parameter .*weight.* modified in place",
                  lambda: same(r.result(), ref, ("outs", "grads"), "head weight changed"), "head weight changed")


def test_parameter_storage_replaced_while_a_forward_is_alive():
    """p.data = p.data.clone() with a forward alive: the next forward raises (the programs would have to be rebuilt under a live
    lease) and keeps raising until the live output is dropped; then forward and backward work again on rebuilt programs, and the
    .grad tensors left from before -- views of the OLD flat buffer, foreign to the new one -- are added into like AccumulateGrad
    does: grad = old + (the whole gradient of the new backward), one fp32 add per element, so the reference is exactly
    g(job 0 alone) + g(job 1 alone).  For a parameter with ONE application that is also the serial run's value, bit for bit; for a
    list-multiplied block it is not (the serial run adds the applications into the slice one by one, ((old + b1) + b2) + b3,
    where a foreign .grad gets old + ((b1 + b2) + b3): same terms, another rounding), which is why only the former are held to
    the serial run here."""
    s0 = SHAPES["pool"][0]
    jobs = (J(s0, 7), J(s0, 8))
    r = Run("pool")
    r.f(0, jobs[0])
    r.b(0)
    r.f(2, jobs[1])                                  # alive
    p = _conv_weight("pool", r.m)
    p.data = p.data.clone()
    for _ in range(2):
        with pytest.raises(RuntimeError, match="waiting for its backward"):
            r.m(_input(s0, 8))
    r.drop(2)
    r.f(1, jobs[1])
    r.b(1)
    res = r.result()
    g0, g1 = serial("pool", jobs[:1], (0,)).grads, serial("pool", jobs[1:], (0,)).grads
    ser = serial("pool", jobs, (0, 1))
    same(res, ser, ("outs",), "after the storage of a parameter was replaced")
    # applications per ConvBlock, from the engine's own step list
    apps = {}
    for op, m, _ in r.eng.steps:
        for cb in ([m] if op == "conv" else m):
            apps[id(cb.conv.weight)] = apps.get(id(cb.conv.weight), 0) + 1
    owner = {id(q): apps[id(ci.mod.conv.weight)] for ci in r.eng.convs for q in ci.params}
    once = 0
    for k, q in r.m.named_parameters():
        same_tensor(res.grads[k], g0[k] + g1[k], "old .grad + new gradient: %s" % k)
        if owner.get(id(q), 1) == 1:
            same_tensor(res.grads[k], ser.grads[k], "serial value: %s" % k)
            once += 1
    assert 0 < once < len(res.grads) and max(apps.values()) == 4


def test_backward_after_parameter_storage_replaced_raises():
    """The live forward's own backward is refused as well: its launch lists name the old storage.  Nothing is launched."""
    s0 = SHAPES["pool"][0]
    r = Run("pool")
    r.f(0, J(s0, 7))
    p = _conv_weight("pool", r.m)
    p.data = p.data.clone()
    with pytest.raises(RuntimeError, match="new storage.*forward again"):
        r.b(0)
    assert not any(q.busy for q in r.programs())
    assert all(q.grad is None for q in r.m.features.parameters())


# ---- belongs with it ------------------------------------------------------------------------------------------------------------
def test_lease_released_when_backward_raises():
    """An exception thrown on the host inside run_backward (a stage-done callback that raises) hands the program back (the
    `finally:` of _EngineFn.backward); the next forward reuses it and, after zero_grad, gives the gradients of a clean run."""
    s0 = SHAPES["pool"][0]
    jobs = (J(s0, 7),)
    r = Run("pool")
    r.f(0, jobs[0])

    def boom(stage):
        raise RuntimeError("stage hook failed at %d" % stage)

    r.eng.on_stage_done = boom
    with pytest.raises(RuntimeError, match="stage hook failed"):
        r.b(0)
    r.eng.on_stage_done = None
    progs = r.programs()
    assert len(progs) == 1 and not progs[0].busy
    r.m.zero_grad(set_to_none=True)
    r.f(0, jobs[0])
    r.b(0)
    assert r.programs() == progs
    same(r.result(), serial("pool", jobs, (0,)), ("outs", "grads"), "after a backward that raised")
