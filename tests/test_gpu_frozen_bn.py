"""-m gpu: training on frozen BatchNorm statistics (model.train(); features.eval()) -- the new kernels against formulas and fp64, the
drop-in modules against tests/frozen_bn_ref.py (the bf16 mirror's eval forward with an explicit frozen-statistics backward, pinned
to fp32 autograd by tests/test_frozen_bn_cpu.py), the bit identities of the mode, and the Trainer.

Bounds (engine vs the bf16 restatement): the ones the same conv kernels meet in train mode -- TIGHT (2e-3) for one ConvBlock,
TIGHT_BLK (3e-2) for a stage, and for the 2x3x64x64 nets tests/test_gpu_model.py's whole-network rules: output 3e-2, gradient cosine
min 0.8 / median 0.95 (test_net), and per-tensor projection coefficient, per-tensor norm ratio and per-stage median projection
(test_net_full_size_vs_mirror).  The constants of the latter, NET_GRAD_SCALE / NET_STAGE_MEDIAN, are measured at 224x224 and batch 32
(>= 1568 samples per channel) and do not carry over to 8 .. 2048 samples per channel, where the eval forward already differs from the
restatement by 2e-3 in y (ReLU-mask flips) and one conv.weight projection measures 1.07 at cosine 0.998; so the same rule is
re-measured at this size, per case and parameter suffix, 1.5x the worst: NET_FROZEN_SCALE / NET_FROZEN_STAGE_MEDIAN below.
MEASURED on an MI355X: one ConvBlock <= 2.1e-6, stages <= 4.3e-5, nets y <= 2.1e-3, cosine min 0.996, projection 0.955 .. 1.083."""
import contextlib
import ctypes
import gc
import io

import numpy as np
import pytest
import torch

import cases as C
import frozen_bn_ref as R
from cases import O
from gpu_util import bits_equal, guarded
from mnasnet_pytorch_amd import _lib as L
from test_oracle_golden import prim_state

pytestmark = pytest.mark.gpu
EPS = 1e-5
FILL32 = 0x7FA5A5A5          # gpu_util.guarded's canary pattern


@pytest.fixture(autouse=True)
def _leave_no_device_memory():
    """An Engine and its module reference each other, so a model dropped at the end of a test frees its scratch tables (> 1 GB for
    the whole network) only when the cycle collector runs; tests that run later in the same process budget their peak memory."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def rl2(a, b):
    a = torch.as_tensor(np.asarray(a)).double().flatten()
    b = torch.as_tensor(np.asarray(b)).double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).cuda()


# ---- the table kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chans", [[8], [24], [40], [1920], [(8, 24, 40, 1920)[j % 4] for j in range(60)]],
                         ids=["n1_C8", "n1_C24", "n1_C40", "n1_C1920", "n60_mixed"])
def test_frozen_tables(chans):
    lib = L.load()
    n = len(chans)
    par, bufs, host = [], [], []
    for j, Cn in enumerate(chans):
        gamma, beta = 1.0 + 0.2 * _rand((Cn,), 10 * j + 1), 0.1 * _rand((Cn,), 10 * j + 2)
        rm, rv = 0.1 * _rand((Cn,), 10 * j + 3), 1.0 + 0.3 * _rand((Cn,), 10 * j + 4).abs()
        rv[(3 * j + 5) % Cn] = 0.0                                   # a dead channel: invstd = 1/sqrt(eps)
        view, check = guarded((8, Cn), torch.float32)
        par.append((gamma, beta, rm, rv))
        bufs.append((view, check))
        host.append((gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), view.data_ptr(), Cn, EPS))
    descs = torch.frombuffer(bytearray(bytes((L.MnasBnFrozenDesc * n)(*host))), dtype=torch.uint8).cuda()
    snap = [[t.clone() for t in p] for p in par]
    L.check(lib.mnas_bn_frozen_tables(descs.data_ptr(), n, L.cur_stream()), "bn_frozen_tables")
    assert lib.mnas_bn_frozen_tables(None, n, L.cur_stream()) == L.EINVAL and lib.mnas_bn_frozen_tables(descs.data_ptr(), 0, L.cur_stream()) == L.EINVAL
    for j, Cn in enumerate(chans):
        gamma, beta, rm, rv = par[j]
        view, check = bufs[j]
        check("frozen table %d (C=%d)" % (j, Cn), written=False)     # nothing outside the block
        raw = view.view(torch.int32)
        assert bool((raw[7] == FILL32).all()), "row 7 written"
        assert not bool((raw[:7] == FILL32).any()), "a channel of rows 0..6 not written"
        ev = torch.full((8, Cn), float("nan"), device="cuda")
        L.check(lib.mnas_bn_fwd_finalize(None, 0, Cn, 0.0, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), None,
                                         0.1, EPS, 0, ev.data_ptr(), L.cur_stream()), "bn_fwd_finalize")
        bits_equal(view[0], ev[0], "row 0 (s) vs the eval finalize")
        bits_equal(view[1], ev[1], "row 1 (t) vs the eval finalize")
        # rows 2..6 by their fp32 formulas (IEEE division and square root, as numpy's)
        invstd = np.float32(1.0) / np.sqrt(rv.cpu().numpy() + np.float32(EPS), dtype=np.float32)
        s = gamma.cpu().numpy() * invstd
        bits_equal(view[2].cpu(), torch.from_numpy(s), "row 2 (c1 = s)")
        bits_equal(view[2], view[0], "row 2 vs row 0")
        bits_equal(view[3:5].cpu(), torch.zeros(2, Cn), "rows 3, 4 (+0)")
        bits_equal(view[5], rm, "row 5 (running mean)")
        bits_equal(view[6].cpu(), torch.from_numpy(invstd), "row 6 (invstd)")
        assert float(view[6].max()) == float(np.float32(1.0) / np.sqrt(np.float32(EPS)))
        for a, b in zip(par[j], snap[j]):
            bits_equal(a, b, "parameter / buffer of descriptor %d" % j)


# ---- the finalize twins ------------------------------------------------------------------------------------------------------------
def _post_inputs(Cn, nparts, seed):
    partial = _rand((2, Cn, nparts), seed)
    bnbuf = _rand((8, Cn), seed + 1)
    old = [_rand((Cn,), seed + 2 + k) for k in range(3)]             # dgamma, dbeta, dbias before the launch
    S1, S2 = partial[0].double().sum(1), partial[1].double().sum(1)
    return partial, bnbuf, old, (S2, S1, bnbuf[0].double() * S1)


def _check_sums(outs, olds, sums, what):
    """every gradient = fl(old + fl(S)): within one fp32 rounding (2^-23 relative) of the accumulated value, S in fp64 on the device"""
    for name, got, old, S in zip(("dgamma", "dbeta", "dbias"), outs, olds, sums):
        want = (old.double() if old is not None else 0.0) + S.float().double()
        err = (got.double() - want).abs()
        bound = 2.0 ** -23 * want.abs()
        assert bool((err <= bound).all()), (what, name, float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("nparts", [1, 3, 256, 257, 1024])
@pytest.mark.parametrize("Cn", [8, 24, 576])
def test_bn_bwd_finalize_frozen(Cn, nparts):
    """stand-alone twin; nparts <= 256: one wave per channel, above: one block per channel"""
    lib = L.load()
    for acc in (0, 1):
        partial, bnbuf, old, sums = _post_inputs(Cn, nparts, 100 + acc)
        before = bnbuf.clone()
        outs = []
        for o in old:
            view, check = guarded((Cn,), torch.float32)
            if acc:
                view.copy_(o)
            outs.append((view, check))
        L.check(lib.mnas_bn_bwd_finalize_frozen(partial.data_ptr(), nparts, Cn, bnbuf.data_ptr(), outs[0][0].data_ptr(),
                                                outs[1][0].data_ptr(), outs[2][0].data_ptr(), acc, L.cur_stream()), "finalize_frozen")
        for view, check in outs:
            check("bn_bwd_finalize_frozen C=%d nparts=%d accumulate=%d" % (Cn, nparts, acc))
        _check_sums([v for v, _ in outs], old if acc else [None] * 3, sums, (Cn, nparts, acc))
        bits_equal(bnbuf, before, "bnbuf")
    assert lib.mnas_bn_bwd_finalize_frozen(None, nparts, Cn, bnbuf.data_ptr(), None, None, None, 1, L.cur_stream()) == L.EINVAL


@pytest.mark.parametrize("nparts", [3, 1024, 1025])
def test_bn_bwd_finalize_frozen_brackets(nparts):
    """dgamma, dbeta and dbias inside the brackets of bounds_se.bn_bwd_finalize_intervals (fp64 on the fp32 table as given).  Up to
    1024 partials every fp32 accumulator of bn_partial_sums holds one term and the bracket is _check_sums' one rounding; 1025 is
    the first table with two terms in an accumulator, which _check_sums' exact-sum model does not describe."""
    from bounds_se import bn_bwd_finalize_intervals
    from intervals import check_interval
    lib = L.load()
    Cn = 24
    for acc in (0, 1):
        partial, bnbuf, old, _ = _post_inputs(Cn, nparts, 500 + acc)
        outs = [o.clone() if acc else torch.full((Cn,), float("nan"), device="cuda") for o in old]
        L.check(lib.mnas_bn_bwd_finalize_frozen(partial.data_ptr(), nparts, Cn, bnbuf.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                outs[2].data_ptr(), acc, L.cur_stream()), "finalize_frozen")
        base = [o.cpu() if acc else None for o in old]
        ivs = bn_bwd_finalize_intervals(partial.cpu(), 1.0, bnbuf.cpu(), base[0], base[1], frozen=True, dbias0=base[2])
        for name, got in zip(("dgamma", "dbeta", "dbias"), outs):
            r = check_interval(got.cpu(), ivs[name], "bn_bwd_finalize_frozen nparts %d accumulate %d %s" % (nparts, acc, name),
                               "BatchNorm backward finalize")
            print("bn_bwd_finalize_frozen nparts %d accumulate %d %s error / bound %.3f" % (nparts, acc, name, r))


def _wg_task(kind, seed):
    """(MnasPostWgrad fields, partial, grad, (nsplit, Co, Ci, taps, dw), the gradient before the launch on the host): a
    single-level weight-gradient reduction, dense 1x1 or depthwise 3x3"""
    dims = (5, 8, 16, 1, 0) if kind == "pw" else (7, 24, 1, 9, 1)
    nsplit, Co, Ci, taps, dw = dims
    total = Co * taps if dw else Co * Ci * taps
    partial, grad = _rand((nsplit, total), seed), _rand((total,), seed + 1)
    return (partial.data_ptr(), grad.data_ptr(), nsplit, Co, Ci, taps, dw, 1), partial, grad, dims, grad.cpu().clone()


@pytest.mark.parametrize("nparts", [1, 3, 256, 257, 1024])
@pytest.mark.parametrize("Cn", [8, 24, 576])
def test_bwd_post_frozen(Cn, nparts):
    """merged twin, with and without weight-gradient tasks riding in the launch; those are mnas_bwd_post's, bit for bit.  dgamma,
    dbeta and dbias of every channel inside bounds_se.bn_bwd_finalize_intervals of the table as given and bit-equal to the
    standalone mnas_bn_bwd_finalize_frozen's (the same bn_bwd_finalize_body<TPC, true>); the weight gradients inside
    check_sum_bound (M = nsplit, c = 1, the accumulate target the +1).  hard: every channel of the table times a power of two
    2^-20..2^4 and the last channel exact zeros."""
    from bounds_se import bn_bwd_finalize_intervals
    from intervals import check_interval, check_sum_bound
    lib = L.load()
    for tasks, hard in ((False, False), (True, False), (True, True)):
        partial, bnbuf, old, sums = _post_inputs(Cn, nparts, 300 + int(tasks))
        if hard:
            partial *= torch.pow(torch.tensor(2.0), ((torch.arange(Cn) * 7) % 25 - 20).float()).cuda().view(1, -1, 1)
            partial[:, Cn - 1] = 0.0
            S1, S2 = partial[0].double().sum(1), partial[1].double().sum(1)
            sums = (S2, S1, bnbuf[0].double() * S1)
        before = bnbuf.clone()
        outs = []
        for o in old:
            view, check = guarded((Cn,), torch.float32)
            view.copy_(o)
            outs.append((view, check))
        a = L.MnasBwdPostFrozen()
        a.bn_partial, a.bnbuf, a.dgamma, a.dbeta, a.dbias = (partial.data_ptr(), bnbuf.data_ptr(), outs[0][0].data_ptr(),
                                                             outs[1][0].data_ptr(), outs[2][0].data_ptr())
        a.count, a.bn_nparts, a.bn_C = 123.0, nparts, Cn
        ref = L.MnasBwdPost()                 # the same tasks through mnas_bwd_post, no BatchNorm part
        keep = []
        if tasks:
            for slot, kind in (("w1", "pw"), ("w2", "dw")):
                f, p_, g_, dims, init = _wg_task(kind, 400 if kind == "pw" else 500)
                f2, p2, g2, _, _ = _wg_task(kind, 400 if kind == "pw" else 500)
                setattr(a, slot, L.MnasPostWgrad(*f))
                setattr(ref, slot, L.MnasPostWgrad(*f2))
                keep.append((p_, g_, p2, g2, dims, init))
        L.check(lib.mnas_bwd_post_frozen(ctypes.byref(a), L.cur_stream()), "bwd_post_frozen")
        for view, check in outs:
            check("bwd_post_frozen C=%d nparts=%d" % (Cn, nparts))
        _check_sums([v for v, _ in outs], old, sums, (Cn, nparts, tasks))
        bits_equal(bnbuf, before, "bnbuf")
        ivs = bn_bwd_finalize_intervals(partial.cpu(), 1.0, bnbuf.cpu(), old[0].cpu(), old[1].cpu(), frozen=True, dbias0=old[2].cpu())
        alone = [o.clone() for o in old]
        L.check(lib.mnas_bn_bwd_finalize_frozen(partial.data_ptr(), nparts, Cn, bnbuf.data_ptr(), alone[0].data_ptr(), alone[1].data_ptr(),
                                                alone[2].data_ptr(), 1, L.cur_stream()), "finalize_frozen")
        for name, (view, _), one in zip(("dgamma", "dbeta", "dbias"), outs, alone):
            check_interval(view.cpu(), ivs[name], "bwd_post_frozen C=%d nparts=%d hard=%d %s" % (Cn, nparts, hard, name), "fused finalize launch")
            bits_equal(view, one, "%s: fused frozen launch vs mnas_bn_bwd_finalize_frozen" % name)
        if tasks:
            for p_, g_, p2, g2, (nsplit, Co, Ci, taps, dw), init in keep:
                tab, init = p_.cpu().double(), init.double()                   # [nsplit][total]; the target in the gradient's layout
                lay = (lambda v: v.view(taps, Co).t().reshape(-1)) if dw else (lambda v: v.view(Co, taps, Ci).permute(0, 2, 1).reshape(-1))
                check_sum_bound(g_.cpu(), lay(tab.sum(0)) + init, lay(tab.abs().sum(0)) + init.abs(), nsplit, 0, 1,
                                "bwd_post_frozen %s task" % ("dw" if dw else "pw"), None, "fused finalize launch")
            L.check(lib.mnas_bwd_post(ctypes.byref(ref), L.cur_stream()), "bwd_post")
            for p_, g_, p2, g2, _, init in keep:
                bits_equal(g_, g2, "weight gradient of a task in the frozen launch vs mnas_bwd_post")
                assert not torch.equal(g_.cpu(), init)                                     # ... and it was accumulated into
    a = L.MnasBwdPostFrozen()
    a.bn_C, a.bn_nparts = Cn, nparts
    assert lib.mnas_bwd_post_frozen(ctypes.byref(a), L.cur_stream()) == L.EINVAL          # BatchNorm part without its tables


class _FrozenBn:
    """the BatchNorm part of one mnas_bwd_post_frozen launch on test_gpu_bwd_forms._bn_table's "hard" table (channels times
    2^-20..2^4, partial columns times 2^0..2^-7, channels whose sum dz is mean*invstd times their sum dz*xhat, the last channel
    exact zeros): guarded table, bnbuf, dgamma, dbeta and dbias, all three accumulated into"""
    def __init__(self, C_, nparts, seed):
        import test_gpu_bwd_forms as BF
        from gpu_util import rand_bn_coefs
        self.C_, self.nparts = C_, nparts
        self.b = rand_bn_coefs(C_, seed + 1, O)
        self.partial = BF._bn_table(C_, nparts, seed, self.b, "hard")
        self.bp, self.pchk = guarded((2, C_, nparts), torch.float32)
        self.bp.copy_(self.partial.cuda())
        self.bnbuf, self.bchk = guarded((8, C_), torch.float32)
        self.bnbuf.copy_(self.b.cuda())
        self.old = [O.det_uniform((C_,), seed + 2 + k) for k in range(3)]
        self.outs = []
        for o in self.old:
            view, check = guarded((C_,), torch.float32)
            view.copy_(o.cuda())
            self.outs.append((view, check))

    def fill(self, a):
        a.bn_partial, a.bnbuf = self.bp.data_ptr(), self.bnbuf.data_ptr()
        a.dgamma, a.dbeta, a.dbias = (v.data_ptr() for v, _ in self.outs)
        a.count, a.bn_nparts, a.bn_C = 123.0, self.nparts, self.C_

    def check(self, what):
        """guards; bnbuf bitwise untouched; every channel of dgamma, dbeta, dbias inside bn_bwd_finalize_intervals(frozen) of the
        table as given and bit-equal to mnas_bn_bwd_finalize_frozen (the same bn_bwd_finalize_body<64 | 256, true>)"""
        from bounds_se import bn_bwd_finalize_intervals
        from intervals import check_interval
        self.pchk(what + " partial")
        self.bchk(what + " bnbuf")
        bits_equal(self.bnbuf.cpu(), self.b, what + ": bnbuf")
        ivs = bn_bwd_finalize_intervals(self.partial, 1.0, self.b, self.old[0], self.old[1], frozen=True, dbias0=self.old[2])
        alone = [o.clone().cuda() for o in self.old]
        bn2 = self.b.clone().cuda()
        L.check(L.load().mnas_bn_bwd_finalize_frozen(self.bp.data_ptr(), self.nparts, self.C_, bn2.data_ptr(), alone[0].data_ptr(),
                                                     alone[1].data_ptr(), alone[2].data_ptr(), 1, L.cur_stream()), "finalize_frozen")
        worst = 0.0
        for name, (view, chk), one in zip(("dgamma", "dbeta", "dbias"), self.outs, alone):
            chk("%s %s" % (what, name))
            worst = max(worst, check_interval(view.cpu(), ivs[name], "%s %s" % (what, name), "fused finalize launch (frozen)"))
            bits_equal(view, one, "%s %s: fused frozen launch vs mnas_bn_bwd_finalize_frozen" % (what, name))
        return worst


def _post_frozen(lib, bn, w1=None, w2=None):
    a = L.MnasBwdPostFrozen()
    bn.fill(a)
    for slot, w in (("w1", w1), ("w2", w2)):
        if w is not None:
            partial, grad, nsplit, Co, Ci, taps, dw, level = w
            setattr(a, slot, L.MnasPostWgrad(L.ptr(partial), L.ptr(grad), nsplit, Co, Ci, taps, dw, level))
    L.check(lib.mnas_bwd_post_frozen(ctypes.byref(a), L.cur_stream()), "bwd_post_frozen")


@pytest.mark.parametrize("C_", [1, 3, 4, 5])
@pytest.mark.parametrize("bn_nparts", [1, 256, 257, 1025])
def test_bwd_post_frozen_mapping(C_, bn_nparts):
    """k_bwd_post_frozen's own mapping of workgroups to the three parts, as test_gpu_bwd_forms.test_bwd_post_mapping holds
    k_bwd_post's: the frozen BatchNorm part on the hard table (C = 1, 3, 4, 5: the `c >= C` return in a partial last workgroup
    of bn_bwd_finalize_body<64, true>; above 256 partials one workgroup per channel; 1025: two terms per fp32 accumulator)
    beside w1 alone, beside w2 alone (w1 at level 0), beside both in either order (108, 5 and 24 x 3 workgroups), and beside a
    level 2 and then a level 3 task in either slot.  Every output inside its bracket and bit-equal to the standalone entry."""
    import test_gpu_bwd_forms as BF
    lib = L.load()
    what = "frozen mapping C=%d nparts=%d" % (C_, bn_nparts)
    empty = (None, None, 0, 0, 0, 0, 0, 0)
    A = lambda tab="scaled": BF._Wg(5, 24, 16, 9, 0, 210, tab)            # 3456 outputs: 108 workgroups
    B = lambda tab="scaled": BF._Wg(130, 16, 1, 9, 1, 212, tab)           # 144 outputs: 5 workgroups
    T2 = lambda tab: BF._Wg(300, 16, 48, 1, 0, 214, tab)                  # 768 outputs: 24 x 3 workgroups at level 2, 24 at level 3
    worst = 0.0
    for name, use in (("w1 only", "a-"), ("w2 only", "-b"), ("w1 + w2", "ab"), ("w2 + w1", "ba")):
        w = {"a": A(), "b": B()}
        slots = [empty if ch == "-" else w[ch].slot(1) for ch in use]
        bn = _FrozenBn(C_, bn_nparts, 220)
        _post_frozen(lib, bn, w1=slots[0], w2=slots[1])
        worst = max(worst, bn.check("%s, %s: bn" % (what, name)))
        for ch in use.replace("-", ""):
            worst = max(worst, w[ch].check("%s, %s: %s" % (what, name, ch.upper())))
    for slot2, slot3 in (("w1", "w2"), ("w2", "w1")):
        for tab in ("sparse", "scaled"):
            t2, a, b = T2(tab), A(), B()
            bn = _FrozenBn(C_, bn_nparts, 222)
            _post_frozen(lib, bn, **{slot2: t2.slot(2), slot3: a.slot(1)})
            worst = max(worst, bn.check("%s, level 2 in %s: bn" % (what, slot2)), a.check("%s, level 2 in %s: A" % (what, slot2)))
            bn = _FrozenBn(C_, bn_nparts, 224)
            _post_frozen(lib, bn, **{slot3: t2.slot(3), slot2: b.slot(1)})
            worst = max(worst, bn.check("%s, level 3 in %s: bn" % (what, slot3)), b.check("%s, level 3 in %s: B" % (what, slot3)),
                        t2.check("%s, level 2 in %s then 3 in %s (%s)" % (what, slot2, slot3, tab)))
    print("%s: worst error / bound %.3f" % (what, worst))


# Scale agreement per tensor at whole-network scope, test_gpu_model.py's rule (NET_GRAD_SCALE / NET_STAGE_MEDIAN) re-measured for
# 2x3x64x64: bounds on |projection coefficient - 1| and |norm ratio - 1| per parameter suffix, {case: {suffix: (projection, norm
# ratio)}}, and on |median projection of a stage's tensors - 1|, each 1.5x the MEASURED worst (MI355X; runs are bit-identical):
#   ccfF     bn.weight    projection 0.9549 .. 1.0823, norm ratio 0.9565 .. 1.0842      stage medians 0.9579 .. 1.0194
#            bn.bias                 0.9565 .. 1.0437             0.9589 .. 1.0464
#            conv.weight             0.9553 .. 1.0705             0.9569 .. 1.0719
#            conv.bias               0.9563 .. 1.0436             0.9586 .. 1.0458
#   ccfT     bn.weight               0.9910 .. 1.0166             0.9915 .. 1.0168      stage medians 0.9969 .. 1.0012
#            bn.bias                 0.9913 .. 1.0055             0.9921 .. 1.0058
#            conv.weight             0.9965 .. 1.0080             0.9967 .. 1.0088
#            conv.bias               0.9954 .. 1.0054             0.9956 .. 1.0056
#   ccfF_se  every tensor, the squeeze-excite MLP's included ("": any suffix): |projection - 1| <= 2.213e-5, |norm ratio - 1| <=
#            2.212e-5 (features.0.bn.weight); every stage median prints as 1.00000 (|. - 1| < 5e-6)
NET_FROZEN_SCALE = {
    "ccfF": {"bn.weight": (0.124, 0.127), "bn.bias": (0.066, 0.070), "conv.weight": (0.106, 0.108), "conv.bias": (0.066, 0.069)},
    "ccfT": {"bn.weight": (0.025, 0.026), "bn.bias": (0.0131, 0.0119), "conv.weight": (0.012, 0.0132), "conv.bias": (0.0081, 0.0084)},
    "ccfF_se": {"": (3.4e-5, 3.4e-5)},
}
NET_FROZEN_STAGE_MEDIAN = {"ccfF": 0.064, "ccfT": 0.0047, "ccfF_se": 7.5e-6}


# ---- the modules against the frozen reference -----------------------------------------------------------------------------------
def _buffers(m):
    return {k: v.clone() for k, v in m.named_buffers()}


def _assert_buffers(m, snap, when):
    for k, v in m.named_buffers():
        if v.dtype.is_floating_point:
            bits_equal(v, snap[k], "%s after %s" % (k, when))
        else:
            assert torch.equal(v, snap[k]), "%s after %s" % (k, when)      # num_batches_tracked


@pytest.mark.parametrize("name", sorted(C.PRIMITIVES))
def test_convblock_frozen(name):
    from mnasnet_pytorch_amd import ConvBlock
    from test_gpu_model import TIGHT, fill
    cin, cout, k, s, p, grp, N, H, W = C.PRIMITIVES[name]
    m = ConvBlock(cin, cout, kernel_size=k, stride=s, padding=p, groups=grp)
    fill(m, name)
    m = m.cuda().eval()
    snap = _buffers(m)
    x0 = C.det_input((N, cin, H, W))
    x = x0.cuda().requires_grad_(True)
    y = m(x)
    cot = C.cotangent(tuple(y.shape))
    (y * cot.cuda()).sum().backward()
    _assert_buffers(m, snap, "forward + backward")
    spec = O.ConvSpec("cb", cin, cout, k, s, p, grp)
    r = R.run([("conv", spec)], prim_state(name, spec), x0, cot, need_dx=True)
    errs = {"y": rl2(y.detach().cpu(), r["y"]), "dx": rl2(x.grad.cpu(), r["dx"])}
    for kk, pp in m.named_parameters():
        assert pp.grad is not None, kk
        errs[kk] = rl2(pp.grad.cpu(), r["grads"]["cb." + kk])
    print(name, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert float(m.conv.bias.grad.abs().max()) > 0
    for kk, e in errs.items():
        assert e < TIGHT, (kk, e)


@pytest.mark.parametrize("name", sorted(C.STAGES))
def test_stage_frozen(name):
    """shared block: `layers` applications accumulate into one set of gradients, conv.bias included"""
    from test_gpu_model import TIGHT_BLK, _stage_setup
    m, prog, st, shp = _stage_setup(name, 0.1)
    m.eval()
    snap = _buffers(m)
    x0 = C.det_input(shp)
    x = x0.cuda().requires_grad_(True)
    y = m(x)
    cot = C.cotangent(tuple(y.shape))
    (y * cot.cuda()).sum().backward()
    _assert_buffers(m, snap, "forward + backward")
    r = R.run(prog, st, x0, cot, need_dx=True)
    errs = {"y": rl2(y.detach().cpu(), r["y"]), "dx": rl2(x.grad.cpu(), r["dx"])}
    for kk, pp in m.named_parameters():
        errs[kk] = rl2(pp.grad.cpu(), r["grads"][kk])
        if kk.endswith("conv.bias"):
            assert float(pp.grad.abs().max()) > 0, kk
    print(name, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert len(errs) == 2 + 16
    for kk, e in errs.items():
        assert e < TIGHT_BLK, (kk, e)


@pytest.mark.parametrize("ccf,se", [(False, 0.0), (True, 0.0), (False, 0.25)], ids=["ccfF", "ccfT", "ccfF_se"])
def test_net_frozen(ccf, se, request):
    from mnasnet_pytorch_amd import Mnasnet
    from test_gpu_model import _grad_agreement, _stage_medians
    st = O.init_state(ccf, C.STATE_SEED, proj_gamma=0.1, se_ratio=se)
    m = Mnasnet(cut_channels_first=ccf, se_ratio=se)
    m.load_state_dict(st)
    m = m.cuda()
    m.train()
    m.features.eval()
    snap = _buffers(m)
    x0 = C.det_input((2, 3, 64, 64))
    y = m(x0.cuda())
    cot = C.cotangent(tuple(y.shape))
    (y * cot.cuda()).sum().backward()
    _assert_buffers(m, snap, "forward + backward")
    on_load = {}
    for lst in m.features._engine().programs.values():
        for prog_ in lst:
            for rec in prog_._se_records.values():
                on_load[(prog_.N, rec.h2.H, rec.h2.W, rec.se.channels)] = bool(rec.kseg)
    assert bool(on_load) == bool(se)
    prog, _ = O.build_program(ccf, se_ratio=se)
    r = R.run(prog, st, x0, cot, se_on_load=(lambda *a: on_load[a]) if se else None)
    e_y = rl2(y.detach().cpu(), r["y"])
    grads = {kk: p.grad.cpu() for kk, p in m.named_parameters()}
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())
    agree = {}
    for kk, gv in grads.items():                    # test_gpu_model._grad_agreement, conv.bias included (not zero in this mode)
        a, b = gv.double().flatten(), r["grads"][kk].double().flatten()
        agree[kk] = {"rel": float((a - b).norm() / (b.norm() + 1e-30)), "cos": float((a @ b) / (a.norm() * b.norm() + 1e-30)),
                     "proj": float(a @ b) / (float(b @ b) + 1e-60), "ratio": float(a.norm() / (b.norm() + 1e-30)), "n": a.numel()}
    assert set(_grad_agreement(grads, r["grads"])) == {kk for kk in agree if not kk.endswith("conv.bias")}
    coss = [v["cos"] for v in agree.values()]
    wr = max(agree.items(), key=lambda kv: kv[1]["rel"])
    med = _stage_medians(agree)
    print("frozen net ccf=%s se=%s: y %.4f; cosine min %.4f median %.4f; worst rel-L2 %.4f (%s)"
          % (ccf, se, e_y, min(coss), float(np.median(coss)), wr[1]["rel"], wr[0]))
    case = request.node.callspec.id
    scale = NET_FROZEN_SCALE[case]
    by_suffix = {}
    for kk, v in agree.items():
        by_suffix.setdefault(next(sfx for sfx in scale if kk.endswith(sfx)), {})[kk] = v
    assert set(by_suffix) == set(scale)
    bad = []
    for suffix, sel in by_suffix.items():
        wp = max(sel.items(), key=lambda kv: abs(kv[1]["proj"] - 1.0))
        wn = max(sel.items(), key=lambda kv: abs(kv[1]["ratio"] - 1.0))
        print("    %-11s projection in [%.4f, %.4f], worst |.-1| %.3e (%s, %d elements); norm ratio in [%.4f, %.4f], worst |.-1| %.3e (%s)"
              % (suffix or "(all)", min(v["proj"] for v in sel.values()), max(v["proj"] for v in sel.values()), abs(wp[1]["proj"] - 1.0),
                 wp[0], wp[1]["n"], min(v["ratio"] for v in sel.values()), max(v["ratio"] for v in sel.values()),
                 abs(wn[1]["ratio"] - 1.0), wn[0]))
        bp, br = scale[suffix]
        bad += [(kk, round(v["proj"], 5), round(v["ratio"], 5)) for kk, v in sel.items()
                if abs(v["proj"] - 1.0) > bp or abs(v["ratio"] - 1.0) > br]
    print("    per-stage median projection: " + "  ".join("features.%s %.5f" % kv for kv in sorted(med.items())))
    # the plain eval forward of the same model: the same values, squeeze-excite included (there the frozen program materialises
    # a*s for the blocks whose project conv has no gate-on-load backward at this size, where plain inference gates on load)
    with torch.no_grad():
        m.eval()
        y_eval = m(x0.cuda())
    bits_equal(y.detach(), y_eval, "tracked frozen forward vs the no-grad eval forward")
    if se:
        eval_on_load = {(p_.N, rec.h2.H, rec.h2.W, rec.se.channels): bool(rec.kseg) for lst in m.features._engine().programs.values()
                        for p_ in lst if not p_.training for rec in p_._se_records.values()}
        assert set(eval_on_load) == set(on_load) and eval_on_load != on_load, (on_load, eval_on_load)      # ... in both forms
    assert e_y < 3e-2
    assert min(coss) > 0.8 and np.median(coss) > 0.95
    assert not bad, bad
    assert all(abs(v - 1.0) <= NET_FROZEN_STAGE_MEDIAN[case] for v in med.values()), med
    for kk in grads:
        if kk.endswith("conv.bias"):
            assert float(grads[kk].abs().max()) > 0, kk


# ---- bit identities ----------------------------------------------------------------------------------------------------------------
def test_frozen_forward_is_the_eval_forward_and_runs_are_bit_identical():
    from mnasnet_pytorch_amd import Mnasnet
    m = Mnasnet(cut_channels_first=False)
    m.load_state_dict(O.init_state(False, C.STATE_SEED, proj_gamma=0.1))
    m = m.cuda().eval()
    snap = _buffers(m)
    x0 = C.det_input((2, 3, 64, 64)).cuda()
    with torch.no_grad():
        y_eval = m(x0)
    eng = m.features._engine()
    assert [k[3] for k in eng.programs] == [False]                       # plain inference: the eval program
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        assert sorted((k[3], k[7]) for k in eng.programs) == [(False, False), (True, True)]       # tracked: the frozen program
        bits_equal(y.detach(), y_eval, "tracked frozen forward vs the no-grad eval forward")
        _assert_buffers(m, snap, "forward")
        (y * C.cotangent(tuple(y.shape)).cuda()).sum().backward()
        _assert_buffers(m, snap, "backward")
        runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not any(p.busy for lst in eng.programs.values() for p in lst)
    # a forward whose graph is dropped hands its program back; a no-grad forward has nothing to run backward through
    for _ in range(6):
        y = m(x0)                                                        # (tracked through the parameters: no input gradient)
        del y
    assert sorted(len(lst) for lst in eng.programs.values()) == [1, 1, 1]


# ---- Trainer ------------------------------------------------------------------------------------------------------------------------
def _frozen_trainer(native):
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_train import _no_dropout, build
    torch.manual_seed(11)
    m = build("512", proj_gamma=0.1).train()
    _no_dropout(m)
    m.freeze_bn()
    tr = Trainer(m, lr=1e-3)
    tr.native_step = native
    return m, tr


def test_trainer_frozen_step():
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = torch.tensor([1, 3, 5, 7]).cuda()
    res = {}
    for native in (True, False):
        m, tr = _frozen_trainer(native)
        assert (tr._native_head() is not None) == native
        tr.optimizer.zero_grad()
        loss = tr.forward_backward(x, t)
        res[native] = (float(loss), tr.flat_g.clone(), sum(p.numel() for p in tr.head_params))
    (l_n, g_n, nh), (l_m, g_m, _) = res[True], res[False]
    # both paths run the same launch lists for the features and the same head kernels.  The loss and dL/dlogits come from
    # mnas_head_cross_entropy on one path and from ATen's log_softmax / nll_loss on the other, an fp32 round-off apart, and the head's
    # weight gradients inherit it (MEASURED: rel-L2 9.9e-8).  The features receive the head's input gradient rounded to bf16, which
    # is the same on both paths here, so the engine part is bit-equal.
    print("native vs module path: loss %.9g / %.9g; head part rel-L2 %.3e; engine part: %d of %d elements differ"
          % (l_n, l_m, rl2(g_n[:nh].cpu(), g_m[:nh].cpu()), int((g_n[nh:] != g_m[nh:]).sum()), g_n.numel() - nh))
    assert abs(l_n - l_m) <= 1e-5 * abs(l_m)
    assert torch.equal(g_n[nh:], g_m[nh:])
    assert rl2(g_n[:nh].cpu(), g_m[:nh].cpu()) < 1e-6

    m, tr = _frozen_trainer(True)
    snap = _buffers(m)
    # two forward_backward calls sum (an fp32 value added to itself is exact)
    tr.optimizer.zero_grad()
    tr.forward_backward(x, t)
    g1 = tr.flat_g.clone()
    bits_equal(g1, g_n, "a second trainer from the same seed")
    tr.forward_backward(x, t)
    print("two calls vs 2 x one call: rel-L2 %.3e, bit-equal: %s" % (rl2(tr.flat_g.cpu(), 2 * g1.cpu()), torch.equal(tr.flat_g, 2 * g1)))
    assert rl2(tr.flat_g.cpu(), (2 * g1).cpu()) < 1e-6
    _assert_buffers(m, snap, "forward_backward")
    # one Adam step moves every conv.bias (its gradient is exactly zero under batch statistics, and Adam leaves such a value alone)
    biases = {k: p.detach().clone() for k, p in m.features.named_parameters() if k.endswith("conv.bias")}
    assert len(biases) == 27
    loss = tr.step(x, t)
    assert np.isfinite(float(loss))
    _assert_buffers(m, snap, "Trainer.step")
    for k, p in m.features.named_parameters():
        if k.endswith("conv.bias"):
            assert float((p.detach() - biases[k]).abs().max()) > 0, k
    assert m.training and not any(mod.training for mod in m.features.modules()) and all(mod.training for mod in m.classifier.modules())

    # validate afterwards: the reference's loop by hand gives the same counts and loss; modes and buffers come back as they were
    from test_gpu_metrics import _hand_loop, _val_batches
    batches = _val_batches(2)
    ref = _hand_loop(m, batches)
    rec = tr.validate(batches)
    assert rec.correct == ref.correct and (rec.samples, rec.steps) == (16, 2)
    assert abs(rec.loss.avg - ref.loss.avg) <= 2e-5 * max(1.0, abs(ref.loss.avg))
    assert m.training and not any(mod.training for mod in m.features.modules()) and all(mod.training for mod in m.classifier.modules())
    _assert_buffers(m, snap, "validate")
    assert np.isfinite(float(tr.step(x, t)))                    # and the frozen step goes on

    # a subtree in mixed modes is still refused, on both paths
    m.features[0].bn.train()
    for native in (True, False):
        tr.native_step = native
        with pytest.raises(NotImplementedError, match="mixed train/eval"):
            tr.forward_backward(x, t)
