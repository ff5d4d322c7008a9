"""-m gpu: the frozen stage prefix (FineTuneModelPool.freeze(upto=k), Engine.first_trainable_step, LaunchPlan first_trainable).

The backward of a model whose leading stages are frozen ends at the first trainable layer.  Everything behind the boundary runs the
launches of the full program, so outputs, BatchNorm buffers and every trainable gradient are compared BITWISE with a run that has
nothing frozen; the handful of launches that only a truncated program of the bench configuration contains are replayed standalone
with their production integers against fp64."""
import contextlib
import gc
import io

import pytest
import torch

import cases as C
from cases import O
from gpu_util import L, relerr
from test_gpu_kernels import TOL_F32
from test_gpu_train import _no_dropout, build

pytestmark = pytest.mark.gpu

SHAPE = (3, 3, 64, 96)          # non-square; the final map is 2 x 3


@pytest.fixture(autouse=True)
def _leave_no_device_memory():
    """An Engine and its module reference each other: a model dropped at the end of a test frees its scratch tables (several GB for
    the whole network) only when the cycle collector runs, and tests that run later in the same process budget their peak memory."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _stage_first(eng):
    first = {}
    for i, (_, _, st) in enumerate(eng.steps):
        first.setdefault(st, i)
    first[max(first) + 1] = len(eng.steps)
    return first


def _model(ccf=False, **kw):
    from mnasnet_pytorch_amd import FineTuneModelPool, Mnasnet
    torch.manual_seed(5)
    m = FineTuneModelPool(Mnasnet(cut_channels_first=ccf, **kw), "mnasnet", 10, "512")
    if not kw:
        m.load_state_dict({**O.init_state(ccf, C.STATE_SEED, proj_gamma=0.1), **O.init_head_state("512", 10, C.STATE_SEED)})
    m = m.cuda().train()
    _no_dropout(m)
    return m


def _module_step(m, x, target):
    """one forward + backward on the module path; (logits, buffers, gradients)"""
    m.zero_grad(set_to_none=True)
    out = m(x)
    loss = torch.nn.CrossEntropyLoss()(out, target)
    assert loss.grad_fn is not None
    loss.backward()
    torch.cuda.synchronize()
    return (out.detach().clone(), {k: b.clone() for k, b in m.named_buffers()},
            {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()})


def _programs(eng):
    return [p for lst in eng.programs.values() for p in lst]


def _compare_with_full(m, k, x, target, state, full, loose=()):
    """reload `state`, freeze(upto=k), one step: everything bitwise against `full` except the parameters named in `loose`, whose
    measured relerr is returned"""
    eng = m.features._engine()
    first = _stage_first(eng)
    m.load_state_dict(state)
    m.freeze(upto=k)
    out, bufs, grads = _module_step(m, x, target)
    f_out, f_bufs, f_grads = full
    assert torch.equal(out, f_out), k
    for name, b in bufs.items():
        assert torch.equal(b, f_bufs[name]), (k, name)
    frozen = {"features.%d." % i for i in range(k)}
    measured = {}
    for name, g in grads.items():
        if any(name.startswith(f) for f in frozen):
            assert g is None, (k, name)
        elif name in loose:
            measured[name] = relerr(g, f_grads[name])
        else:
            assert g is not None and torch.equal(g, f_grads[name]), (k, name)
    prog = [p for p in _programs(eng) if p.first_trainable == first[k]]
    assert len(prog) == 1 and [st for st, _, _ in prog[0].bwd_segments] == list(range(7, k - 1, -1)), k
    assert not prog[0].busy
    return measured


@pytest.mark.parametrize("fused_pw", [False, True], ids=["default", "pw_fused_everywhere"])
@pytest.mark.parametrize("ccf", [False, True], ids=["ccf0", "ccf1"])
def test_same_launches_same_bits(ccf, fused_pw):
    """freeze(upto=k), k = 1..7, on the module path against the run with everything trainable.  pw_fused_everywhere:
    pw_fused_min_pixels = 0 makes the full program run the fused 1x1 backward wherever the bench-size step does; the boundary block's
    expand conv then takes k_wgrad instead, and that one weight gradient is held to 2 * TOL_F32 (both kernels are held to TOL_F32
    against fp64) instead of bitwise."""
    m = _model(ccf)
    eng = m.features._engine()
    if fused_pw:
        eng.pw_fused_min_pixels = 0
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x = C.det_input(SHAPE).cuda()
    target = torch.tensor([1, 7, 4]).cuda()
    full = _module_step(m, x, target)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in full[2].values()) and bool(torch.isfinite(full[0]).all())
    assert [p.first_trainable for p in _programs(eng)] == [0]
    first = _stage_first(eng)
    names = {id(p): n for n, p in m.named_parameters()}
    for k in range(1, 8):
        loose = ()
        op, mods, _ = eng.steps[first[k]]
        if fused_pw and op == "block":
            loose = (names[id(mods[0].conv.weight)],)         # the boundary block's expand conv
        measured = _compare_with_full(m, k, x, target, state, full, loose)
        for name, e in measured.items():
            print("k=%d ccf=%d %s: k_wgrad at the boundary vs the fused 1x1 backward, relerr %.3e" % (k, ccf, name, e))
            assert e < 2 * TOL_F32, (k, name, e)
    assert len(eng.programs) == 8                            # one program per boundary


def test_trainer_native_step_with_a_frozen_prefix():
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input(SHAPE).cuda()
    target = torch.tensor([1, 7, 4]).cuda()

    def make(k):
        m = build("512", proj_gamma=0.1).train()
        _no_dropout(m)
        if k:
            m.freeze(upto=k)
        return m, Trainer(m, lr=1e-3, weight_decay=1e-2)

    ends = []
    for rep in range(2):
        m, tr = make(4)
        eng = tr.engine
        first = _stage_first(eng)
        n_head = tr.flat_g.numel() - eng.grad_numel
        a = n_head + min(eng.stage_ranges[s][0] for s in range(4))          # the frozen stages are the tail of the flat layout
        assert a == n_head + max(eng.stage_ranges[s][1] for s in range(4, 8))
        assert sum(p.numel() for c in list(m.features)[:4] for p in c.parameters()) == tr.flat_g.numel() - a
        assert tr._native_head() is not None and tr._frozen_prefix() == first[4]
        p0 = tr.flat_p.clone()
        for step in range(3):
            loss = tr.step(x, target)
            assert loss.grad_fn is None and not loss.requires_grad and bool(torch.isfinite(loss))
            torch.cuda.synchronize()
            assert torch.equal(tr.flat_p[a:], p0[a:]), "a frozen weight moved (step %d)" % step
            assert not bool(tr.flat_g[a:].any()), "a kernel wrote a frozen gradient (step %d)" % step
            assert bool(tr.flat_g[n_head:a].any())
            if step == 0 and rep == 0:
                g1 = tr.flat_g[:a].clone()
                bufs1 = {k: b.clone() for k, b in m.named_buffers()}
        assert not torch.equal(tr.flat_p[:a], p0[:a])
        progs = _programs(eng)
        assert [p.first_trainable for p in progs] == [first[4]] and [st for st, _, _ in progs[0].bwd_segments] == [7, 6, 5, 4]
        ends.append(tr.flat_p.clone())
        if rep == 0:
            # a twin with nothing frozen: the same launches behind the boundary, so the same bits after one step
            m2, tr2 = make(0)
            tr2.step(x, target)
            torch.cuda.synchronize()
            assert torch.equal(tr2.flat_g[:a], g1)
            assert bool(tr2.flat_g[a:].any())
            for k, b in m2.named_buffers():
                assert torch.equal(b, bufs1[k]), k
            del m2, tr2
    assert torch.equal(ends[0], ends[1])
    # unfreeze(): the next step runs the full program and the stem trains again
    with contextlib.redirect_stdout(io.StringIO()):
        m.unfreeze()
    w0 = m.features[0].conv.weight.detach().clone()
    nkeys = len(eng.programs)
    tr.step(x, target)
    torch.cuda.synchronize()
    assert len(eng.programs) == nkeys + 1 and sorted(p.first_trainable for p in _programs(eng)) == [0, first[4]]
    assert not torch.equal(m.features[0].conv.weight.detach(), w0)
    # what is no stage prefix keeps the module path
    m.freeze(upto=2)
    assert tr._native_head() is not None
    bn_w = [p for n, p in m.features[5].named_parameters() if n.endswith("bn.weight")][0]
    bn_w.requires_grad = False
    assert tr._native_head() is None and tr._frozen_prefix() is None
    w5 = bn_w.detach().clone()
    tr.step(x, target)                                           # the module path takes the truncated program too
    torch.cuda.synchronize()
    assert torch.equal(bn_w.detach(), w5) and first[2] in [p.first_trainable for p in _programs(eng)]
    m.freeze(upto=0)
    for p in m.features[3].parameters():
        p.requires_grad = False
    assert tr._native_head() is None
    with contextlib.redirect_stdout(io.StringIO()):
        m.freeze()
    assert tr._native_head() is None
    m.freeze(upto=8)
    assert tr._native_head() is None                             # all features frozen: the module path, which skips the backward


def test_frozen_statistics_with_a_frozen_prefix():
    m = _model(False)
    m.freeze_bn()
    assert not m.features.training and m.classifier.training
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x = C.det_input(SHAPE).cuda()
    target = torch.tensor([1, 7, 4]).cuda()
    full = _module_step(m, x, target)
    for name, b in full[1].items():
        assert torch.equal(b, state[name]), name                  # frozen statistics: no buffer moves
    bias = [n for n in full[2] if n.endswith("conv.bias") and int(n.split(".")[1]) >= 3]
    assert bias and all(bool(full[2][n].any()) for n in bias)     # not cancelled by batch statistics here
    _compare_with_full(m, 3, x, target, state, full)
    eng = m.features._engine()
    assert sorted((k[7], k[8]) for k in eng.programs) == [(True, 0), (True, _stage_first(eng)[3])]


def test_squeeze_excite_with_a_frozen_prefix():
    m = _model(False, kernel_size=5, se_ratio=0.25)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x = C.det_input(SHAPE).cuda()
    target = torch.tensor([1, 7, 4]).cuda()
    full = _module_step(m, x, target)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in full[2].values())
    assert any(".se." in n for n in full[2])
    _compare_with_full(m, 3, x, target, state, full)


# ---- the launches only a truncated program of the bench configuration contains ------------------------------------------------------
def _post_census(prog):
    """WGRAD_FINALIZE and BWD_POST launches by (opcode, integers, pointer slots present)"""
    seen = set()
    for _, arr, n in prog.bwd_segments:
        for j in range(n):
            o = arr[j]
            if o.opcode in (L.OP_WGRAD_FINALIZE, L.OP_BWD_POST):
                seen.add((o.opcode, L.op_ints(o), tuple(bool(o.p[s]) for s in range(16))))
    return seen


def _census(prog):
    import test_gpu_bwd_forms as BF
    import test_gpu_fwd_forms as FF
    fw, fin = {}, set()
    FF._census(prog, fw, fin)
    return set(fw), fin, set(BF._census(prog)), _post_census(prog)


@pytest.fixture(scope="module")
def bench_remainders():
    """{k: census of the bench configuration's program with the boundary at stage k, minus the full program's census}, k = 1..4.
    The programs are built, not run, one at a time (each holds 5-10 GB)."""
    from mnasnet_pytorch_amd import FineTuneModelPool, load_model
    from mnasnet_pytorch_amd.train_step import Trainer
    N, HW = 256, 224
    with contextlib.redirect_stdout(io.StringIO()):
        base = load_model("mnasnet")
    m = FineTuneModelPool(base, "mnasnet", 1000, "512").cuda().train()
    tr = Trainer(m, lr=1e-3)
    eng = tr.engine
    eng.ensure_setup(torch.device("cuda"))
    eng._check_modes()
    first = _stage_first(eng)
    full = _census(eng.program(N, HW, HW, True, False, True, False))
    eng.reset_programs()
    out = {}
    for k in range(1, 5):
        m.freeze(upto=k)
        assert tr._frozen_prefix() == first[k]
        prog = eng.program(N, HW, HW, True, False, True, False, first_trainable=tr._frozen_prefix())
        out[k] = tuple(a - b for a, b in zip(_census(prog), full))
        del prog
        eng.reset_programs()
    del tr, eng, m, base
    gc.collect()
    torch.cuda.empty_cache()
    return out


def _PTRS(*on):
    return tuple(s in on for s in range(16))


_VIRT_DY = (("dy.y", True), ("virt", True))
# k -> (CONV_WGRAD integers, its WGRAD_FINALIZE, the BWD_POST launch left with only its level-3 half) / the DW_BWD integers
_EXPECT = {
    1: dict(dw=(256, 112, 112, 32, 3, 2048, 0, 0, 0)),
    2: dict(wgrad=(256, 112, 112, 16, 112, 112, 48, 1, 1, 1, 0, 512), fin=(512, 48, 16, 1), post_w2=(768, 48, 1, 9, 1, 3)),
    3: dict(wgrad=(256, 56, 56, 24, 56, 56, 72, 1, 1, 1, 0, 512), fin=(512, 72, 24, 1), post_w2=(512, 72, 1, 25, 1, 3)),
    4: dict(wgrad=(256, 28, 28, 40, 28, 28, 240, 1, 1, 1, 0, 256), fin=(256, 240, 40, 1)),
}


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_boundary_launches_at_production_integers(k, bench_remainders):
    """BASELINE configs[1] (ccf=False, head '512', bs 256, 224x224): what the program with the boundary at stage k launches that the full
    program does not -- k = 2, 3, 4: k_wgrad on the boundary block's expand conv (virtual input, dy formed on load) at a pixel count
    where the full step runs the fused 1x1 backward, its WGRAD_FINALIZE, and the depthwise reduction's level-3 half flushed in a
    BWD_POST launch of its own; k = 1: the fused depthwise sweep without the fused reduce -- each replayed standalone with guarded
    buffers against fp64 on the device."""
    import test_gpu_bwd_forms as BF
    import test_gpu_fwd_forms as FF
    lib = L.load()
    fw, fin, bw, post = bench_remainders[k]
    e = _EXPECT[k]
    want_fw = {(L.OP_CONV_WGRAD, e["wgrad"], _VIRT_DY)} if "wgrad" in e else set()
    want_fin = {e["fin"]} if "fin" in e else set()
    want_bw = set()
    if "dw" in e:
        want_bw = {(L.OP_DW_BWD, e["dw"], (("dy.y", True), ("gin", True), ("red", False), ("virt", True), ("wpartial", True)))}
    want_post = set()
    if "fin" in e:
        want_post.add((L.OP_WGRAD_FINALIZE, e["fin"] + (1,), _PTRS(0, 1)))
    if "post_w2" in e:
        want_post.add((L.OP_BWD_POST, (0,) * 8 + e["post_w2"], _PTRS(6, 7)))
    assert (fw, fin, bw, post) == (want_fw, want_fin, want_bw, want_post)
    gen = torch.Generator(device="cuda").manual_seed(2028 + k)
    torch.cuda.reset_peak_memory_stats()
    for _, ints, flags in fw:
        print("k=%d CONV_WGRAD %s: %s" % (k, ints, FF._replay_wgrad(ints, dict(flags), gen)))
    for _, ints, flags in bw:
        print("k=%d DW_BWD %s: %s" % (k, ints, BF._replay_dw(ints, dict(flags), gen, ints[0])))
    torch.cuda.synchronize()
    for opc, ints, _ in post:
        if opc == L.OP_WGRAD_FINALIZE:          # accumulate = 1 onto a gradient that is already there, as the step runs it
            nsplit, Co, Ci, taps, acc = ints
            w = BF._Wg(nsplit, Co, Ci, taps, 0, 300 + k)
            L.check(lib.mnas_wgrad_finalize(L.ptr(w.part), nsplit, Co, Ci, taps, L.ptr(w.grad), acc, L.cur_stream()), "wgrad_finalize")
            w.check("k=%d wgrad_finalize %s" % (k, ints))
        else:                                    # the launch that carried level 2 beside a BatchNorm part is the full program's
            nsplit, Co, Ci, taps, dw, level = ints[8:]
            assert (Ci, dw, level) == (1, 1, 3)
            w = BF._Wg(nsplit, Co, Ci, taps, dw, 310 + k)
            BF._post(lib, w1=w.slot(2))
            BF._post(lib, w2=w.slot(3))
            w.check("k=%d bwd_post with only its level-3 half %s" % (k, ints))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.cuda.max_memory_allocated() / 2 ** 30 < 20
