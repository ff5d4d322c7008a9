"""CPU (no GPU needed): every launch plan the planner can emit passes tests/plan_verify.py -- extents inside their tensors, no
unordered conflicting accesses, no read of an undefined byte, every reduce table read whole from its one producer, forward buffers
alive until their backward readers, every trainable gradient range targeted once per application -- and the verifier reports each
of ten injected faults, alone, at the op and slot it was injected.  The access model (tests/plan_access.py) is held to the kernels
by tests/test_gpu_plan_access.py."""
import pytest
import torch

import make_launch_plan_golden as G
import plan_access as A
import plan_verify as V
from mnasnet_pytorch_amd import Mnasnet
from mnasnet_pytorch_amd import _lib as L
from mnasnet_pytorch_amd.engine import Engine

CONFIGS = G.configs()
CPU = torch.device("cpu")


def build_golden(cfg, side):
    """(engine, program, model) of one golden configuration, with or without the side stream"""
    return G.build_program(cfg, CPU, {"use_side_stream": True, "new_event": V.event_counter()} if side else {})


def build_default(N, H, W, side=False, frozen_bn=False, first_trainable=0, **switches):
    """the default net's training program at one shape; first_trainable: a step index or a function of the engine"""
    m = Mnasnet().train()
    eng = Engine(m.features)
    for k, v in switches.items():
        assert hasattr(eng, k)
        setattr(eng, k, v)
    if side:
        eng.use_side_stream = True
        eng.new_event = V.event_counter()
    eng.ensure_setup(CPU)
    first = first_trainable(eng) if callable(first_trainable) else first_trainable
    prog = eng.program(N, H, W, True, False, True, False, frozen_bn=frozen_bn, first_trainable=first)
    return eng, prog, m


def show(findings):
    return "\n".join("%s[%d] %s.%s: %s -- %s" % f for f in findings)


def where(findings):
    return {(f.list, f.index, f.slot) for f in findings}


# ---- the model's key set ----------------------------------------------------------------------------------------------------------
def test_model_covers_every_pointer_slot():
    assert A.check_model_covers_slots() == ([], [])
    assert A.EXEMPT == ()


def test_key_check_sees_a_missing_slot_and_a_new_opcode():
    access = {opc: dict(slots) for opc, slots in A.ACCESS.items()}
    del access[L.OP_DW_BWD]["red_bn"]
    assert A.check_model_covers_slots(access) == ([(L.OP_DW_BWD, "red_bn")], [])
    slots = dict(L.OP_SLOTS)
    slots[99] = (("n",), (), ("src", None, "dst"))
    assert A.check_model_covers_slots(None, slots) == ([(99, "dst"), (99, "src")], [])


# ---- no findings on any plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [False, True], ids=["main", "side"])
@pytest.mark.parametrize("name,full,cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_golden_configurations(name, full, cfg, side):
    eng, prog, m = build_golden(cfg, side)
    found = V.verify(eng, V.PlanView(prog))
    assert not found, show(found)


def _middle_stage_start(eng):
    stages = sorted({st for _, _, st in eng.steps})
    mid = stages[len(stages) // 2]
    return next(i for i, (_, _, st) in enumerate(eng.steps) if st == mid)


EXTRA = [("frozen_bn", dict(N=256, H=224, W=224, frozen_bn=True)),
         ("frozen_bn_2x32x32", dict(N=2, H=32, W=32, frozen_bn=True)),
         ("first0", dict(N=256, H=224, W=224, first_trainable=0)),
         ("first_middle_stage", dict(N=256, H=224, W=224, first_trainable=_middle_stage_start)),
         ("first_last_step", dict(N=256, H=224, W=224, first_trainable=lambda eng: len(eng.steps) - 1)),
         ("first_len_steps", dict(N=256, H=224, W=224, first_trainable=lambda eng: len(eng.steps))),
         ("frozen_bn_first_middle_stage", dict(N=256, H=224, W=224, frozen_bn=True, first_trainable=_middle_stage_start))]
EXTRA += [("batch%d" % n, dict(N=n, H=224, W=224)) for n in (1, 2, 33, 256)]
EXTRA += [("plane%dx%d" % hw, dict(N=16, H=hw[0], W=hw[1])) for hw in ((32, 32), (57, 75), (224, 224), (192, 256), (512, 384))]


@pytest.mark.parametrize("side", [False, True], ids=["main", "side"])
@pytest.mark.parametrize("name,kw", EXTRA, ids=[e[0] for e in EXTRA])
def test_default_net_modes_batches_and_planes(name, kw, side):
    eng, prog, m = build_default(side=side, **kw)
    found = V.verify(eng, V.PlanView(prog))
    assert not found, show(found)
    if name == "first_len_steps":
        assert not prog.bwd_segments


# ---- the checker bites: ten injected faults ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main_plan():
    return build_default(256, 224, 224)


@pytest.fixture(scope="module")
def side_plan():
    return build_default(256, 224, 224, side=True, join_stages=set(range(64)))


def sync_all(view):
    view.bwd_all = [o for _, ops in view.segments for o in ops]


def find_ops(view, pred):
    return [(lst, j, o) for lst, ops in view.lists() for j, o in enumerate(ops) if pred(o)]


def set_field(o, name, v):
    kind, k = L._SLOT[o.opcode][name]
    getattr(o, kind)[k] = v


def ptr(o, name):
    return int(L.op_field(o, name) or 0)


def test_clean_plans(main_plan, side_plan):
    for eng, prog, _ in (main_plan, side_plan):
        assert V.verify(eng, V.PlanView(prog)) == []


@pytest.mark.parametrize("delta", [1, -1])
@pytest.mark.parametrize("field,slot", [("bn_nparts", "bn_partial"), ("w1.nsplit", "w1.partial")])
def test_injection_1_finalize_rows_differ_from_the_producer(main_plan, field, slot, delta):
    eng, prog, _ = main_plan
    view = V.PlanView(prog)
    hits = find_ops(view, lambda o: o.opcode == L.OP_BWD_POST and L.op_field(o, "bn_C") > 0 and L.op_field(o, "w1.level") == 1
                    and L.op_field(o, "bn_nparts") > 1 and L.op_field(o, "w1.nsplit") > 1)
    lst, j, o = hits[len(hits) // 2]
    set_field(o, field, L.op_field(o, field) + delta)
    sync_all(view)
    found = V.verify(eng, view)
    assert where(found) == {(lst, j, slot)}, show(found)
    assert "writer" in found[0].kind or "undefined" in found[0].kind


def test_injection_2_producer_writes_the_table_whose_reduce_has_not_run(main_plan):
    eng, prog, _ = main_plan
    view = V.PlanView(prog)
    # a launch that runs the second level of table T (written two producers ago) and the first level of table T1 (the producer just
    # before it): point that producer, this launch's first task and the second level that follows it at T -- what a rotation over
    # two buffers would hand out.  The producer then overwrites the folded rows of T before their second level has read them.
    for lst, ops in view.lists():
        for j, o in enumerate(ops):
            if not (o.opcode == L.OP_BWD_POST and L.op_field(o, "w2.level") == 3 and L.op_field(o, "w1.level") == 2):
                continue
            t, t1 = ptr(o, "w2.partial"), ptr(o, "w1.partial")
            prod = [k for k in range(j) if ops[k].opcode in (L.OP_PW_BWD, L.OP_DW_BWD) and ptr(ops[k], "wpartial") == t1]
            nxt = [k for k in range(j + 1, len(ops)) if ops[k].opcode == L.OP_BWD_POST and L.op_field(ops[k], "w2.level") == 3]
            if t == t1 or not prod or not nxt or ptr(ops[nxt[0]], "w2.partial") != t1:
                continue
            set_field(ops[prod[-1]], "wpartial", t)
            set_field(o, "w1.partial", t)
            set_field(ops[nxt[0]], "w2.partial", t)
            sync_all(view)
            found = V.verify(eng, view)
            assert where(found) == {(lst, j, "w2.partial")}, show(found)
            assert "writer" in found[0].kind
            return
    pytest.fail("the plan has no two consecutive two-level reductions")


def _last_segment_side_ops(view):
    st, ops = view.segments[-1]
    return "bwd%d" % st, ops, [j for j, o in enumerate(ops) if int(o.i[L.OP_STREAM_SLOT]) == 1]


def test_injection_3_join_removed(side_plan):
    eng, prog, _ = side_plan
    view = V.PlanView(prog)
    lst, ops, side = _last_segment_side_ops(view)
    j = max(k for k, o in enumerate(ops) if o.opcode == L.OP_EVENT_WAIT and int(o.i[L.OP_STREAM_SLOT]) == 0)
    del ops[j]
    sync_all(view)
    fins = [k for k in side if ops[k].opcode == L.OP_WGRAD_FINALIZE]
    assert len(fins) == 1                                   # (the stem's segment: one weight gradient on the side stream)
    found = V.verify(eng, view)
    assert where(found) == {(lst, fins[0], "grad")}, show(found)
    assert found[0].kind == "order"


def test_injection_4_fork_removed(side_plan):
    eng, prog, _ = side_plan
    view = V.PlanView(prog)
    lst, ops, side = _last_segment_side_ops(view)
    j = max(k for k in side if ops[k].opcode == L.OP_EVENT_WAIT)
    del ops[j]
    sync_all(view)
    patch = view.patch_x_bwd
    assert patch[1] == j + 1
    view.patch_x_bwd = (patch[0], j, patch[2])
    assert ops[j].opcode == L.OP_STEM_WGRAD
    found = V.verify(eng, view)
    # what the main stream wrote after the previous fork: the incoming gradient and the coefficients just finalised
    assert where(found) == {(lst, j, "dy.g"), (lst, j, "dy.coef")}, show(found)
    assert {f.kind for f in found} == {"order"}


def test_injection_5_op_deleted(main_plan):
    eng, prog, _ = main_plan
    view = V.PlanView(prog)
    st, ops = view.segments[0]
    j = next(k for k, o in enumerate(ops) if o.opcode == L.OP_BN_BWD_REDUCE)
    assert j > view.patch_gout[1]
    del ops[j]
    sync_all(view)
    assert ops[j].opcode == L.OP_BWD_POST
    found = V.verify(eng, view)
    assert where(found) == {("bwd%d" % st, j, "bn_partial")}, show(found)


def test_injection_6_two_dependent_ops_swapped(main_plan):
    eng, prog, _ = main_plan
    view = V.PlanView(prog)
    fins = [j for j, o in enumerate(view.fwd) if o.opcode == L.OP_BN_FWD_FINALIZE]
    j = fins[len(fins) // 2]
    assert ptr(view.fwd[j - 1], "stats") == ptr(view.fwd[j], "partial")
    view.fwd[j - 1], view.fwd[j] = view.fwd[j], view.fwd[j - 1]
    found = V.verify(eng, view)
    # the finalize reads the previous layer's table; what it leaves in the block is then what the next launches read: they are
    # ordered and defined, so the one finding is the read
    assert where(found) == {("fwd", j - 1, "partial")}, show(found)


@pytest.mark.parametrize("scratch", ["scratch_red", "scratch_wgrad2"])
def test_injection_7_scratch_one_row_short(main_plan, scratch):
    eng, prog, _ = main_plan
    view = V.PlanView(prog)
    base = getattr(eng, scratch).data_ptr()
    owners = V._Owners(eng, prog, {})
    uses = []               # (list, index, slot, bytes from the table's base)
    for lst, ops in view.lists():
        for j, o in enumerate(ops):
            if o.opcode in (L.OP_EVENT_RECORD, L.OP_EVENT_WAIT):
                continue
            for slot, mode, start, n in A.op_accesses(o, eng.lib, owners.peek):
                if base <= start < base + getattr(eng, scratch).numel() * 4:
                    uses.append((lst, j, slot, start + n - base))
    need = max(u[3] for u in uses)
    short = torch.empty(need - 4, dtype=torch.uint8)          # the largest table of the plan, less its last float
    for lst, ops in view.lists():
        for o in ops:
            for k in range(16):
                if o.opcode not in (L.OP_EVENT_RECORD, L.OP_EVENT_WAIT) and o.p[k] == base:
                    o.p[k] = short.data_ptr()
    sync_all(view)
    view.extra_owners["scratch_short"] = short
    found = V.verify(eng, view)
    assert where(found) == {(lst, j, slot) for lst, j, slot, end in uses if end == need}, show(found)
    assert all("extent" in f.kind for f in found)


def test_injection_8_forward_buffer_reused_before_its_backward_reader(main_plan):
    eng, prog, _ = main_plan
    view = V.PlanView(prog)
    # the input gradient a project conv's backward writes takes the place of the expand conv's raw output y, same shape, which the
    # expand conv's backward still reads: every launch that names the gradient buffer is renamed (a planner that aliased the two)
    for st, ops in view.segments:
        for j, o in enumerate(ops):
            if o.opcode != L.OP_PW_BWD or not ptr(o, "gin"):
                continue
            gin, nbytes = ptr(o, "gin"), L.op_field(o, "M") * L.op_field(o, "Ci") * 2
            later = [(k, q) for k in range(j + 1, len(ops)) for q in ops[k:k + 1]]
            ys = [ptr(q, "dy.y") for k, q in later if q.opcode == L.OP_PW_BWD and ptr(q, "dy.y")
                  and L.op_field(q, "M") * L.op_field(q, "Co") * 2 == nbytes and ptr(q, "dy.y") != ptr(o, "x.data")]
            if not ys:
                continue
            y = ys[0]
            readers = set()
            for k, q in later:
                for s in range(16):
                    if q.opcode in (L.OP_EVENT_RECORD, L.OP_EVENT_WAIT):
                        continue
                    if q.p[s] == gin:
                        q.p[s] = y
                    # every later read of the buffer is one of a forward buffer that no longer holds the forward's write: those
                    # that wanted y, and those that want the gradient now in its place
                    if q.p[s] == y:
                        readers.add(("bwd%d" % st, k, V.slot_name(q.opcode, s)))
            o.p[L.slot(L.OP_PW_BWD, "gin")] = y
            sync_all(view)
            found = V.verify(eng, view)
            assert readers and where(found) == readers, show(found)
            assert all("liveness" in f.kind for f in found)
            return
    pytest.fail("no project / expand pair found")


def test_injection_9_finalize_retargeted_into_the_neighbouring_parameter(main_plan):
    eng, prog, _ = main_plan
    view = V.PlanView(prog)
    lst, j, o = find_ops(view, lambda o: o.opcode == L.OP_WGRAD_FINALIZE)[0]
    numel = L.op_field(o, "Co") * L.op_field(o, "Ci") * L.op_field(o, "taps")
    set_field(o, "grad", ptr(o, "grad") + 4 * numel)         # the conv bias follows the weight in the flat layout
    sync_all(view)
    found = V.verify(eng, view)
    off = (ptr(o, "grad") - eng.flat_grad.data_ptr()) // 4 - numel
    name = next(n for n, p in eng.root.named_parameters()
                for ci in eng.convs if p is ci.params[0] and ci.gslice[0] == (off, numel))
    # the write is no parameter's range, and the weight it belonged to is left without its launch
    assert where(found) == {(lst, j, "grad"), ("params", -1, name)}, show(found)
    assert all("cover" in f.kind for f in found)


def test_injection_10_patch_gout_on_a_write_slot(main_plan):
    eng, prog, _ = main_plan
    view = V.PlanView(prog)
    st, j, k = view.patch_gout
    assert view.seg(st)[j].opcode == L.OP_POOL_BWD
    view.patch_gout = (st, j, L.slot(L.OP_POOL_BWD, "g"))
    found = V.verify(eng, view)
    assert where(found) == {("bwd%d" % st, j, "g")}, show(found)
    assert found[0].kind == "patch"
