"""CPU (no GPU needed): training on frozen BatchNorm statistics.

* tests/frozen_bn_ref.py (the bf16 restatement the GPU tests compare against) is pinned to fp32 autograd through the oracle's eval
  forward, within what bf16 storage costs -- the bounds tests/test_bf16_mirror.py applies to the train-mode mirror at the same scope
  (one ConvBlock: y 1e-2, gradients 1.2e-1; blocks / stages: y 3e-2, dx 1.2e-1, gradients 0.2; whole network: y 8e-2, gradient
  norms within 0.4 .. 2.5 of the fp32 ones) -- and every case is shown to be LIVE: each ConvBlock output active on 5-95 % of its
  elements and every conv.bias gradient non-zero (the gradient that exists only in this mode).
* the frozen launch plan, built on the CPU like tests/golden/make_launch_plan_golden.py builds the pinned ones: the eval forward
  plus ONE table launch, the train backward with the finalizes replaced by their frozen twins.
* FineTuneModelPool.freeze_bn(): module state that survives model.train(), model.eval() and a pickle round trip."""
import ctypes
import pickle
import re

import numpy as np
import pytest
import torch

import cases as C
import frozen_bn_ref as R
import make_launch_plan_golden as G
from cases import O
from mnasnet_pytorch_amd import _lib as L
from test_oracle_golden import prim_state


def rl2(a, b):
    a = torch.as_tensor(np.asarray(a)).double().flatten()
    b = torch.as_tensor(np.asarray(b)).double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- fp32 autograd through the oracle's eval forward -----------------------------------------------------------------------------
def _leaves(st):
    """fp32 copy of a state dict whose floating tensors require grad; aliases of a shared block stay ONE tensor"""
    memo = {}
    out = {}
    for k, v in st.items():
        if id(v) not in memo:
            memo[id(v)] = v.clone().requires_grad_(True) if (v.dtype.is_floating_point and "running" not in k) else v.clone()
        out[k] = memo[id(v)]
    return out


def _oracle_eval(program, st, x, cot, ccf=None):
    """y, dx, {name: grad} of L = sum(y * cot) in fp32, eval mode; active: the active fraction of every ConvBlock application.
    ccf given: the whole network through oracle.features_forward(train=False) (program only names the ConvBlocks)."""
    ls = _leaves(st)
    before = {k: v.detach().clone() for k, v in ls.items() if "running" in k or "tracked" in k}
    xr = x.clone().requires_grad_(True)
    active = []
    if ccf is not None:
        y = O.features_forward(xr, ls, ccf, False)
    h = xr
    for op, arg in program:                         # the same forward step by step: the ConvBlock outputs for the liveness condition
        if op == "conv":
            h = O.convblock(h, ls, arg, False)
            active.append(float((h > 0).float().mean()))
        else:
            a = h
            for s in arg[:3]:
                a = O.convblock(a, ls, s, False)
                active.append(float((a > 0).float().mean()))
            h = h + a
    if ccf is None:
        y = h
    else:
        assert torch.equal(y.detach(), h.detach())
    (y * cot).sum().backward()
    for k, v in before.items():
        assert torch.equal(ls[k], v), k             # eval mode: the buffers are not touched
    grads = {k: v.grad for k, v in ls.items() if v.dtype.is_floating_point and v.requires_grad}
    return y.detach(), xr.grad, grads, active


def _check_live(name, active, grads):
    assert all(0.05 <= a <= 0.95 for a in active), (name, "active fraction per ConvBlock application", active)
    norms = {k: float(v.norm()) for k, v in grads.items() if k.endswith("conv.bias")}
    assert norms and all(n > 0 for n in norms.values()), (name, norms)
    return min(active), max(active), min(norms.values()), max(norms.values())


@pytest.mark.parametrize("name", sorted(C.PRIMITIVES))
def test_ref_primitive(name):
    cin, cout, k, s, p, grp, N, H, W = C.PRIMITIVES[name]
    spec = O.ConvSpec("cb", cin, cout, k, s, p, grp)
    st = prim_state(name, spec)
    x = C.det_input((N, cin, H, W))
    prog = [("conv", spec)]
    y0 = R.run(prog, st, x)["y"]
    cot = C.cotangent(tuple(y0.shape))
    y, dx, grads, active = _oracle_eval(prog, st, x, cot)
    print(name, "active %.2f..%.2f, |d conv.bias| %.3g..%.3g" % _check_live(name, active, grads))
    snap = {k: v.clone() for k, v in st.items()}
    r = R.run(prog, st, x, cot, need_dx=True)
    assert all(torch.equal(st[k], v) for k, v in snap.items())          # the reference leaves the state alone too
    assert rl2(r["y"], y) < 1e-2
    if cin != 3:
        assert rl2(r["dx"], dx) < 1.2e-1
    for suf in ("conv.weight", "conv.bias", "bn.weight", "bn.bias"):
        e = rl2(r["grads"]["cb." + suf], grads["cb." + suf])
        print("  %-12s rel-L2 %.4f" % (suf, e))
        assert e < 1.2e-1, (suf, e)


def _stage_program(name, proj_gamma=0.1):
    """the stand-alone stage of tests/test_gpu_model.py::_stage_setup as (program, state, input shape)"""
    cin, cout, t, layers, k, reduce, ccf, N, H, W = C.STAGES[name]
    bc = cout if ccf else cin
    conv = O.ConvSpec("sequence.%d" % (0 if ccf else layers), cin, cout, 3, 2 if reduce else 1, 1, 1)
    blk = O._block_specs("sequence.%d" % (1 if ccf else 0), bc, t, k)
    st = {}
    for s_ in [conv] + blk:
        for suf, shp in (("conv.weight", s_.weight_shape()), ("conv.bias", (s_.cout,)), ("bn.weight", (s_.cout,)),
                         ("bn.bias", (s_.cout,)), ("bn.running_mean", (s_.cout,)), ("bn.running_var", (s_.cout,))):
            st[s_.prefix + "." + suf] = O.det_param("%s.%s.%s" % (name, s_.prefix, suf), shp, C.STATE_SEED)
        st[s_.prefix + ".bn.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    st[blk[2].prefix + ".bn.weight"] = st[blk[2].prefix + ".bn.weight"] * proj_gamma
    prog = ([("conv", conv)] if ccf else []) + [("block", blk)] * layers + ([] if ccf else [("conv", conv)])
    return prog, st, (N, cin, H, W)


@pytest.mark.parametrize("name", sorted(C.STAGES))
def test_ref_stage(name):
    prog, st, shp = _stage_program(name)
    x = C.det_input(shp)
    cot = C.cotangent(tuple(R.run(prog, st, x)["y"].shape))
    y, dx, grads, active = _oracle_eval(prog, st, x, cot)
    print(name, "active %.2f..%.2f, |d conv.bias| %.3g..%.3g" % _check_live(name, active, grads))
    r = R.run(prog, st, x, cot, need_dx=True)
    assert rl2(r["y"], y) < 3e-2
    assert rl2(r["dx"], dx) < 1.2e-1
    for kk, gv in r["grads"].items():
        e = rl2(gv, grads[kk])
        print("  %-32s rel-L2 %.4f" % (kk, e))
        assert e < 0.2, (kk, e)


@pytest.mark.parametrize("ccf", [False, True])
def test_ref_net(ccf):
    st = O.init_state(ccf, C.STATE_SEED, proj_gamma=0.1)
    prog, _ = O.build_program(ccf)
    x = C.det_input((2, 3, 64, 64))
    cot = C.cotangent(tuple(R.run(prog, st, x)["y"].shape))
    y, _, grads, active = _oracle_eval(prog, st, x, cot, ccf=ccf)
    lo, hi, nlo, nhi = _check_live("net ccf=%s" % ccf, active, grads)
    print("net ccf=%s: active %.2f..%.2f, |d conv.bias| %.3g..%.3g, smallest running_var %.3g"
          % (ccf, lo, hi, nlo, nhi, min(float(v.min()) for k, v in st.items() if k.endswith("running_var"))))
    assert len(active) == 57
    r = R.run(prog, st, x, cot)
    e = rl2(r["y"], y)
    print("  y rel-L2 %.4f" % e)
    assert e < 0.08
    n, worst = 0, (1.0, None)
    for kk, gv in r["grads"].items():
        ratio = float(gv.double().norm()) / float(grads[kk].double().norm())
        if abs(np.log(ratio)) > abs(np.log(worst[0])):
            worst = (ratio, kk)
        assert 0.4 <= ratio <= 2.5, (kk, ratio)
        n += 1
    print("  gradient norm ratio furthest from 1: %.3f (%s) over %d tensors" % (worst + (n,)))
    assert n == 4 * len({id(s) for op, a in prog for s in ([a] if op == "conv" else a)})


# ---- the frozen launch plan --------------------------------------------------------------------------------------------------
_CONV_FWD = (L.OP_STEM_FWD, L.OP_DW_FWD, L.OP_CONV_GEMM)


def _build(mode, switches=None):
    """(engine, program, model, ops) for ccf False at 2x32x32, built like make_launch_plan_golden.build_program builds the pinned
    plans; mode: "train" / "eval" / "frozen".  ops: [(list tag, opcode, 15 ints, 4 doubles, 16 pointer names)], buffers of the
    program named by shape and dtype only (their numbering follows first use, which differs between the three lists)."""
    from mnasnet_pytorch_amd import Mnasnet
    from mnasnet_pytorch_amd.engine import Engine
    m = Mnasnet(cut_channels_first=False)
    m.train(mode == "train")
    eng = Engine(m.features)
    for k, v in (switches or {}).items():
        assert hasattr(eng, k)
        setattr(eng, k, v)
    eng.ensure_setup(torch.device("cpu"))
    eng.reset_programs()
    if mode == "frozen":
        prog = eng.program(2, 32, 32, True, False, True, False, frozen_bn=True)
    else:
        prog = eng.program(2, 32, 32, mode == "train", False, True, False)
    names = G._Names(eng, prog)

    def nm(ptr):
        return re.sub(r"^b\d+:", "b:", names(ptr))

    ops = []
    for tag, arr, n in [("fwd", prog.fwd_ops, prog.fwd_n)] + [("bwd%d" % st, a, k) for st, a, k in prog.bwd_segments]:
        for j in range(n):
            o = arr[j]
            ops.append((tag, int(o.opcode), tuple(int(v) for v in o.i), tuple(float(v) for v in o.d),
                        tuple(nm(o.p[k]) for k in range(16))))
    return eng, prog, m, ops


def test_frozen_program_arguments():
    from mnasnet_pytorch_amd import Mnasnet
    from mnasnet_pytorch_amd.engine import Engine
    eng = Engine(Mnasnet(cut_channels_first=False).features)
    eng.ensure_setup(torch.device("cpu"))
    a = eng.program(2, 32, 32, True, False, True, False, frozen_bn=True)
    assert a.frozen_bn and eng.program(2, 32, 32, True, False, True, False, frozen_bn=True) is a
    b = eng.program(2, 32, 32, True, False, True)                       # the positional call: the train program, another key
    assert b is not a and not b.frozen_bn
    with pytest.raises(ValueError):
        eng.program(2, 32, 32, False, False, True, False, frozen_bn=True)
    eng.reset_programs()


def test_frozen_plan_forward():
    eng, prog, m, ops = _build("frozen")
    _, _, m_e, ops_e = _build("eval")
    fwd = [o for o in ops if o[0] == "fwd"]
    fwd_e = [o for o in ops_e if o[0] == "fwd"]
    # one table launch right after the weight packing, one descriptor per ConvBlock application
    assert [o[1] for o in fwd[:2]] == [L.OP_PACK_BATCH, L.OP_BN_FROZEN_BATCH]
    assert sum(o[1] == L.OP_BN_FROZEN_BATCH for o in fwd) == 1 and not any(o[1] == L.OP_BN_FWD_FINALIZE for o in fwd)
    napp = sum(o[1] == L.OP_BN_FWD_FINALIZE for o in fwd_e)
    assert napp == 57 == len(prog._records)
    tab = prog.fwd_ops[1]
    assert L.op_field(tab, "n") == napp
    raw = [t for t in prog.keep if t.data_ptr() == L.op_field(tab, "descs")]
    assert len(raw) == 1 and raw[0].numel() == napp * ctypes.sizeof(L.MnasBnFrozenDesc) and ctypes.sizeof(L.MnasBnFrozenDesc) == 48
    descs = (L.MnasBnFrozenDesc * napp).from_buffer_copy(raw[0].numpy().tobytes())
    names = G._Names(eng, prog)
    blocks = set()
    for d, rec in zip(descs, prog._records):
        bn = rec.ci.mod.bn
        assert (d.gamma, d.beta, d.running_mean, d.running_var) == (bn.weight.data_ptr(), bn.bias.data_ptr(),
                                                                    bn.running_mean.data_ptr(), bn.running_var.data_ptr())
        assert names(d.gamma).endswith("bn.weight") and names(d.running_var).endswith("bn.running_var")
        assert d.C == rec.ci.cout == bn.num_features and d.eps == np.float32(bn.eps)
        assert d.bnbuf == rec.out.bn.data_ptr() and tuple(rec.out.bn.shape) == (8, d.C)
        blocks.add(d.bnbuf)
    assert len(blocks) == napp                                  # shared blocks: one coefficient block per APPLICATION
    # everything else is the eval forward: the conv launches (NULL statistics table included) and the glue, slot by slot
    rest = [o for o in fwd if o[1] != L.OP_BN_FROZEN_BATCH]
    rest_e = [o for o in fwd_e if o[1] != L.OP_BN_FWD_FINALIZE]
    assert [o[1] for o in rest] == [o[1] for o in rest_e]
    nconv = 0
    for o, e in zip(rest, rest_e):
        if o[1] == L.OP_PACK_BATCH:
            # legitimately different: `n` and the descriptor table -- a program with a backward also packs the input-gradient layouts
            assert o[2][0] > e[2][0] and o[2][1:] == e[2][1:]
            continue
        assert o[1:] == e[1:], (G.OP_NAMES[o[1]], o, e)
        if o[1] in _CONV_FWD:
            nconv += 1
            assert o[4][L.slot(o[1], "stats")] == "-"
    assert nconv == napp
    eng.reset_programs()


@pytest.mark.parametrize("merge_post", [True, False])
def test_frozen_plan_backward(merge_post):
    sw = {"merge_post": merge_post}
    eng, prog, m, ops = _build("frozen", sw)
    eng_t, prog_t, m_t, ops_t = _build("train", sw)
    bwd = [o for o in ops if o[0] != "fwd"]
    bwd_t = [o for o in ops_t if o[0] != "fwd"]
    twin = {L.OP_BWD_POST_FROZEN: L.OP_BWD_POST, L.OP_BN_BWD_FINALIZE_FROZEN: L.OP_BN_BWD_FINALIZE}
    assert [(o[0], twin.get(o[1], o[1])) for o in bwd] == [(o[0], o[1]) for o in bwd_t]
    assert [st for st, _, _ in prog.bwd_segments] == [st for st, _, _ in prog_t.bwd_segments]
    bias_of = {}            # byte offset of a ConvBlock's bn.weight gradient in the flat buffer -> that of its conv.bias gradient
    for ci in eng.convs:
        bias_of[4 * ci.gslice[2][0]] = 4 * ci.gslice[1][0]
        assert ci.params[1] is ci.mod.conv.bias and ci.params[2] is ci.mod.bn.weight

    def off(name):
        assert name == "flat_grad" or name.startswith("flat_grad+"), name
        return int(name.split("+")[1]) if "+" in name else 0

    ntwin = 0
    for o, t in zip(bwd, bwd_t):
        if o[1] == L.OP_BWD_POST_FROZEN:
            # a mnas_bwd_post launch with a BatchNorm part: same integers, doubles and pointers; `dbias` is the one added slot
            kd = L.slot(o[1], "dbias")
            assert o[2] == t[2] and o[3] == t[3] and o[4][:kd] == t[4][:kd] and t[4][kd] == "-" and o[2][1] > 0
            assert off(o[4][kd]) == bias_of[off(o[4][L.slot(o[1], "dgamma")])]
            ntwin += 1
        elif o[1] == L.OP_BN_BWD_FINALIZE_FROZEN:
            # same integers and pointers + `dbias`; legitimately different: no `count` (d[0]) -- nothing is averaged over the batch
            kd = L.slot(o[1], "dbias")
            assert o[2] == t[2] and o[4][:kd] == t[4][:kd] and t[4][kd] == "-"
            assert o[3] == (0.0,) * 4 and t[3][0] > 0 and t[3][1:] == (0.0,) * 3
            assert off(o[4][kd]) == bias_of[off(o[4][L.slot(o[1], "dgamma")])]
            ntwin += 1
        else:
            assert o[1:] == t[1:], (G.OP_NAMES[o[1]], o, t)          # (a mnas_bwd_post launch without a BatchNorm part included)
            assert o[1] != L.OP_BWD_POST or o[2][1] == 0
    assert ntwin == 57
    eng.reset_programs()
    eng_t.reset_programs()


# ---- FineTuneModelPool.freeze_bn() -------------------------------------------------------------------------------------------
def test_freeze_bn_is_module_state():
    import contextlib
    import copy
    import io
    from mnasnet_pytorch_amd import FineTuneModelPool, load_model
    with contextlib.redirect_stdout(io.StringIO()):
        m = FineTuneModelPool(load_model("mnasnet"), "mnasnet", 10, "512")

    def modes(mod):
        return {x.training for x in mod.modules()}

    assert m.bn_frozen is False and modes(m) == {True}
    assert m.freeze_bn() is m and m.bn_frozen
    assert m.training and modes(m.features) == {False} and modes(m.classifier) == {True} and modes(m.pooling) == {True}
    m.train()                                                   # train.py:419 calls it every epoch
    assert m.training and modes(m.features) == {False} and modes(m.classifier) == {True}
    m.eval()
    assert modes(m) == {False}
    m.train()
    assert modes(m.features) == {False} and modes(m.classifier) == {True}
    assert all(p.requires_grad for p in m.parameters())         # independent of freeze() / unfreeze()
    with contextlib.redirect_stdout(io.StringIO()):
        m.freeze()
        m.unfreeze()
    assert m.bn_frozen and modes(m.features) == {False} and all(p.requires_grad for p in m.parameters())
    for other in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert other.bn_frozen and modes(other.features) == {False} and modes(other.classifier) == {True}
        other.train()
        assert modes(other.features) == {False}
    m.freeze_bn(False)
    assert not m.bn_frozen and modes(m) == {True}
    m.eval()
    m.freeze_bn(False)
    assert modes(m) == {False}                                  # switching it off does not start training an eval-mode model
    m.train()
    assert modes(m) == {True}
