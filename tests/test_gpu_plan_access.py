"""GPU: the access model of tests/plan_access.py held to what the kernels touch.  Small programs are stepped one op at a time through
mnas_run_ops_multi, with a device sync after each op, from two start states that differ in every byte the verifier calls undefined at
start (0x7fc07fc0 words in run A, 0x5a bytes in run B; gaps between the tensors included) and agree in everything else.  Every tensor
the program and the engine own -- parameters, buffers, the flat gradient, packed weights, the six scratch tables, the program's
buffers, the run-time tensors -- lives in one arena with canary gaps, so after each op, in both runs:

  writes           the bytes that changed lie inside the op's declared write extents;
  writes complete  the declared write extents hold the same bytes in both runs (an under-filled extent, or a read of an undefined
                   byte, shows as a difference), so the defined state agrees after every op; at the end the output, dx and the flat
                   gradient are finite and bit-equal;
  reads            run B executes op j with every arena byte outside its declared read and write extents replaced by noise (and put
                   back afterwards): what it writes must not depend on anything it does not declare.

A load that a mask discards cannot be seen this way, and neither can an access outside the arena.  Nothing here provokes a fault: the
fills are data and every launch is the plan's own launch with its own integers."""
import ctypes as C

import pytest
import torch

import make_launch_plan_golden as G
import plan_access as A
import plan_verify as V
from mnasnet_pytorch_amd import Mnasnet
from mnasnet_pytorch_amd import _lib as L
from mnasnet_pytorch_amd.engine import Engine, Program
from mnasnet_pytorch_amd.launch_plan import L_BN_ROWS

pytestmark = pytest.mark.gpu
GAP = 1024               # canary bytes in front of and behind every tensor
SCRATCHES = ("scratch_stats", "scratch_red", "scratch_wgrad", "scratch_wgrad2", "scratch_wgrad3", "scratch_wgrad4")


class Arena:
    """one device allocation that hands out views with canary gaps between them"""

    def __init__(self, nbytes, device):
        self.mem = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.base, self.top = self.mem.data_ptr(), GAP
        self.defined = []           # (first byte, bytes) of what is defined at start

    def alloc(self, shape, dtype, like=None):
        numel = 1
        for s in shape:
            numel *= int(s)
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        start = (self.top + 255) // 256 * 256
        if start + nbytes + GAP > self.mem.numel():
            raise MemoryError("arena too small")
        self.top = start + nbytes + GAP
        t = self.mem[start:start + nbytes].view(dtype).view(tuple(shape))
        if like is not None:
            t.copy_(like)
            self.defined.append((start, nbytes))
        return t


class ArenaProgram(Program):
    """a Program whose own buffers come out of the arena, the coefficient blocks included (undefined, not zeroed)"""

    def __init__(self, arena, *args, **kw):
        self._arena = arena
        super().__init__(*args, **kw)

    def _new(self, shape, dtype=torch.bfloat16):
        t = self._arena.alloc(shape, dtype)
        self.keep.append(t)
        return t

    def _bnbuf(self, C_):
        return self._new((L_BN_ROWS, C_), torch.float32)


CASES = {
    "default_2x32x32": dict(shape=(2, 3, 32, 32)),
    "default_3x40x56": dict(shape=(3, 3, 40, 56)),
    "se_2x32x32": dict(shape=(2, 3, 32, 32), se=0.25),
    "u8_norm_2x32x32": dict(shape=(2, 3, 32, 32), u8=True),
    "frozen_bn_2x32x32": dict(shape=(2, 3, 32, 32), frozen_bn=True),
    "first_trainable_mid_2x32x32": dict(shape=(2, 3, 32, 32), first="middle"),
    "features3_dx_2x24x12x20": dict(shape=(2, 24, 12, 20), subtree=3, need_dx=True),
    "default_2x32x32_side": dict(shape=(2, 3, 32, 32), side=True),
}


def build(case, device):
    """(engine, program, arena, io tensors, model)"""
    torch.manual_seed(1234)
    m = Mnasnet(se_ratio=case.get("se", 0.0)).to(device).train()
    root = m.features if case.get("subtree") is None else m.features[case["subtree"]]
    eng = Engine(root)
    eng.use_side_stream = bool(case.get("side"))
    if case.get("u8"):
        eng.set_input_normalization(G.MEAN, G.STD)
    eng.ensure_setup(device)
    nbytes = sum(getattr(eng, s).numel() * 4 for s in SCRATCHES) + (96 << 20)
    arena = Arena(nbytes, device)
    with torch.no_grad():
        gen = torch.Generator(device="cpu").manual_seed(7)
        for name, b in root.named_buffers():            # running statistics a step away from their initial values
            if b.dtype == torch.float32:
                b.copy_((torch.rand(b.shape, generator=gen) * 0.5 + (0.75 if name.endswith("running_var") else -0.25)).to(device))
        for t in list(root.parameters()) + list(root.buffers()):
            t.data = arena.alloc(t.shape, t.dtype, like=t.data)
    eng.bind_grad_buffer(arena.alloc((eng.grad_numel,), torch.float32, like=torch.zeros(eng.grad_numel, device=device)))
    eng.ensure_setup(device)
    for s in SCRATCHES:
        setattr(eng, s, arena.alloc((getattr(eng, s).numel(),), torch.float32))
    for ci in eng.convs:
        for attr in ("w_fwd", "w_dgrad", "w_tconv"):
            t = getattr(ci, attr, None)
            if t is not None:
                setattr(ci, attr, arena.alloc(t.shape, t.dtype))
    u8 = bool(case.get("u8"))
    aff = eng.input_affine(u8)
    if aff is not None:
        eng._in_aff[(u8, device)] = arena.alloc(aff.shape, aff.dtype, like=aff)
    N, Cin, H, W = case["shape"]
    first = 0
    if case.get("first") == "middle":
        stages = sorted({st for _, _, st in eng.steps})
        first = next(i for i, (_, _, st) in enumerate(eng.steps) if st == stages[len(stages) // 2])
    prog = ArenaProgram(arena, eng, N, H, W, True, bool(case.get("need_dx")), case.get("subtree") is None, u8,
                        frozen_bn=bool(case.get("frozen_bn")), first_trainable=first)
    gen = torch.Generator(device="cpu").manual_seed(11)
    x = (torch.randint(0, 256, (N, Cin, H, W), generator=gen, dtype=torch.uint8) if u8
         else torch.randn((N, Cin, H, W), generator=gen)).to(device)
    io = {"x": arena.alloc(x.shape, x.dtype, like=x),
          "gout": arena.alloc(prog.out_shape, torch.float32, like=torch.randn(prog.out_shape, generator=gen).to(device)),
          "out": arena.alloc(prog.out_shape, torch.float32),
          "dx": arena.alloc((N, Cin, H, W), torch.float32)}
    return eng, prog, arena, io, m


def _mask(arena, ranges):
    m = torch.zeros(arena.mem.numel(), dtype=torch.bool, device=arena.mem.device)
    for start, n in ranges:
        a = start - arena.base
        if 0 <= a and a + n <= m.numel():
            m[a:a + n] = True
    return m


def _first_offsets(mask, limit=4):
    idx = torch.nonzero(mask)[:limit, 0].tolist()
    return idx


@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_kernels_touch_what_the_model_declares(name):
    case, device = CASES[name], torch.device("cuda:0")
    eng, prog, arena, io, m = build(case, device)
    view = V.PlanView(prog)
    assert V.check_patches(eng, view, io) == []             # (applies the run-time pointers to the view's lists)
    owners = V._Owners(eng, prog, io)
    lib, live, base = eng.lib, arena.mem, arena.base

    def whose(off):
        k = owners.find(base + off)
        return "a gap" if k is None else "%s+%d" % (owners.label(k), base + off - owners.ranges[k][0])

    # ---- the two start states: different wherever nothing is defined, the same everywhere else
    defined = _mask(arena, [(base + s, n) for s, n in arena.defined])
    keep = live.clone()
    sa = torch.tensor([0xC0, 0x7F], dtype=torch.uint8, device=device).repeat(live.numel() // 2 + 1)[:live.numel()].clone()
    sb = torch.full_like(live, 0x5A)
    sa = torch.where(defined, keep, sa)
    sb = torch.where(defined, keep, sb)
    noise = torch.randint(0, 256, (live.numel(),), dtype=torch.uint8, device=device, generator=torch.Generator(device=device).manual_seed(3))
    del keep, defined
    streams = (C.c_void_p * 2)(L.cur_stream(), eng.side_stream_handle())
    failed = C.c_int(-1)

    def run(o):
        torch.cuda.synchronize(device)          # (the state was laid out on the current stream; the op may run on the side stream)
        rc = lib.mnas_run_ops_multi(C.byref(o), 1, streams, 2, C.byref(failed))
        torch.cuda.synchronize(device)
        assert rc == 0, "launch refused with code %d" % rc

    problems = []
    for lst, ops in view.lists():
        for j, o in enumerate(ops):
            tag = "%s[%d] %s" % (lst, j, G.OP_NAMES[o.opcode])
            if o.opcode in (L.OP_EVENT_RECORD, L.OP_EVENT_WAIT):
                run(o)
                continue
            accs = A.op_accesses(o, lib, owners.peek)
            wmask = _mask(arena, [(s, n) for _, md, s, n in accs if md in (A.W, A.RW)])
            rwmask = wmask | _mask(arena, [(s, n) for _, md, s, n in accs if md in (A.R, A.RW)])
            # ---- run A
            live.copy_(sa)
            run(o)
            changed = live != sa
            stray = changed & ~wmask
            if bool(stray.any()):
                problems.append("%s (run A) writes outside its declared extents: %s" % (tag, [whose(i) for i in _first_offsets(stray)]))
            sa.copy_(live)
            # ---- run B: everything the op does not declare is noise while it runs
            before = torch.where(rwmask, sb, noise)
            live.copy_(before)
            run(o)
            stray_b = (live != before) & ~wmask
            if bool(stray_b.any()):
                problems.append("%s (run B) writes outside its declared extents: %s" % (tag, [whose(i) for i in _first_offsets(stray_b)]))
            differ = (live != sa) & wmask
            if bool(differ.any()):
                problems.append("%s: its write extents differ between the runs (an extent not filled, or a read the model does not "
                                "declare): %s" % (tag, [whose(i) for i in _first_offsets(differ)]))
            # the next op starts from B's own untouched bytes and, in everything this op wrote, from what run A holds: a problem
            # reported once does not show again at every later reader
            sb = torch.where(wmask | changed, sa, sb)
            del changed, stray, stray_b, differ, before, wmask, rwmask
            if len(problems) >= 20:
                break
        if len(problems) >= 20:
            break
    assert not problems, "\n".join(problems)
    # ---- the results: finite, and the same bits in both runs
    results = {"out": io["out"], "flat_grad": eng.flat_grad}
    if prog.patch_dx is not None:
        results["dx"] = io["dx"]
    live.copy_(sa)
    for what, t in results.items():
        a = t.data_ptr() - base
        n = t.numel() * t.element_size()
        assert bool(torch.isfinite(t).all()), "%s is not finite" % what
        assert torch.equal(sa[a:a + n], sb[a:a + n]), "%s differs between the runs" % what
    assert bool(eng.flat_grad.abs().sum() > 0) and bool(io["out"].abs().sum() > 0)
    eng.reset_programs()
