"""-m gpu: the native classifier head + loss (csrc/mnas_head.hip, mnasnet_pytorch_amd/head.py) against the CPU oracle
(oracle.head_forward_masked / F.cross_entropy, fp32) -- classifiers.py:56-89,107-111 and train.py:277,434-439.
Tolerances: fp32 products over K <= 1000 in a different summation order than ATen's: 2e-5 relative to the tensor's
max; the dropout keep mask must equal the oracle's restatement of the hash bit for bit.  Next to those: per-element bounds for
the three GEMM entry points and brackets for the cross-entropy kernels (bounds_tail.head_gemm_interval, ce_intervals; DESIGN.md
section 6), which see an error in a small element next to a large one."""
import ctypes as Ct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bounds_tail as BT
import cases as C
import gpu_util as G
import intervals as IV
from cases import O
from gpu_util import relerr
from mnasnet_pytorch_amd import _lib as L
from mnasnet_pytorch_amd.head import NativeHead, parse_sequential, _mix

pytestmark = pytest.mark.gpu
TOL = 2e-5


def _lin(N, I, O_, relu, p, seed, x, w, b):
    a = L.MnasHeadLinear()
    a.N, a.I, a.O, a.relu, a.drop_p, a.seed = N, I, O_, int(relu), p, seed
    a.x, a.w, a.b = x.data_ptr(), w.data_ptr(), L.ptr(b)
    return a


def _keep(seed, N, I, p):
    if p == 0:
        return torch.ones(N, I, dtype=torch.bool)
    return torch.from_numpy(O.head_dropout_keep(seed, N * I, p).reshape(N, I))


@pytest.mark.parametrize("N,I,O_", [(256, 320, 512), (37, 320, 1000), (5, 512, 10), (64, 256, 1000), (130, 70, 65)])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.2])
def test_linear_fwd_bwd(N, I, O_, p):
    lib = L.load()
    seed = 0x1234567890ABCDEF ^ (N * 7919 + I)
    x, w, b = O.det_uniform((N, I), 1), O.det_uniform((O_, I), 2) * 0.1, O.det_uniform((O_,), 3)
    dz = O.det_uniform((N, O_), 4)
    u_prev = O.det_uniform((N, I), 5)                         # "input of this layer" as the ReLU mask source
    keep = _keep(seed, N, I, p)
    sc = 1.0 / (1.0 - float(np.float32(p)))
    xd = (x * keep * sc).double()
    xc, wc, bc, dzc, uc = (t.cuda() for t in (x, w, b, dz, u_prev))
    # device mask == oracle restatement
    if p > 0:
        mk = torch.empty(N * I, dtype=torch.uint8, device="cuda")
        L.check(lib.mnas_head_dropout_mask(mk.data_ptr(), N * I, p, seed, L.cur_stream()))
        assert torch.equal(mk.cpu().bool().view(N, I), keep)
        assert abs(float(keep.float().mean()) - (1 - p)) < 0.03
    for relu in (False, True):
        y = torch.full((N, O_), float("nan"), device="cuda")
        a = _lin(N, I, O_, relu, p, seed, xc, wc, bc)
        a.y = y.data_ptr()
        L.check(lib.mnas_head_linear_fwd(Ct.byref(a), L.cur_stream()))
        ref = xd @ w.double().t() + b.double()
        if relu:
            ref = ref.clamp_min(0)
        assert relerr(y.cpu(), ref) < TOL
    # weight / bias gradient, overwrite and accumulate
    for acc in (0, 1):
        dw = torch.full((O_, I), 0.25, device="cuda") if acc else torch.full((O_, I), float("nan"), device="cuda")
        db = torch.full((O_,), -0.5, device="cuda") if acc else torch.full((O_,), float("nan"), device="cuda")
        a = _lin(N, I, O_, False, p, seed, xc, wc, bc)
        a.dz, a.dw, a.db, a.accumulate = dzc.data_ptr(), dw.data_ptr(), db.data_ptr(), acc
        L.check(lib.mnas_head_linear_bwd_w(Ct.byref(a), L.cur_stream()))
        assert relerr(dw.cpu(), dz.double().t() @ xd + (0.25 if acc else 0.0)) < TOL
        assert relerr(db.cpu(), dz.double().sum(0) + (-0.5 if acc else 0.0)) < TOL
    # input gradient with and without the ReLU mask of the layer in front
    for masked in (False, True):
        dx = torch.full((N, I), float("nan"), device="cuda")
        a = _lin(N, I, O_, False, p, seed, xc, wc, bc)
        a.dz, a.dx = dzc.data_ptr(), dx.data_ptr()
        a.relu_mask = uc.data_ptr() if masked else None
        L.check(lib.mnas_head_linear_bwd_x(Ct.byref(a), L.cur_stream()))
        ref = (dz.double() @ w.double()) * keep * sc
        if masked:
            ref = ref * (u_prev > 0)
        assert relerr(dx.cpu(), ref) < TOL


@pytest.mark.parametrize("N,Cn", [(256, 1000), (7, 10), (33, 257)])
def test_cross_entropy(N, Cn):
    lib = L.load()
    x = O.det_uniform((N, Cn), 11) * 4
    t = torch.from_numpy((np.arange(N) * 7 + 3) % Cn).long()
    for ignore in (False, True):
        tt = t.clone()
        if ignore:
            tt[::3] = -100
        xr = x.clone().double().requires_grad_(True)
        ref = F.cross_entropy(xr, tt)
        ref.backward()
        rows = torch.empty(N, device="cuda")
        loss = torch.empty((), device="cuda")
        dl = torch.full((N, Cn), float("nan"), device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        xc, tc = x.cuda(), tt.cuda()
        L.check(lib.mnas_head_cross_entropy(xc.data_ptr(), tc.data_ptr(), N, Cn, -100, rows.data_ptr(),
                                            loss.data_ptr(), dl.data_ptr(), bad.data_ptr(), L.cur_stream()))
        assert abs(float(loss) - float(ref.detach())) < 2e-5 * max(1.0, abs(float(ref.detach())))
        assert relerr(dl.cpu(), xr.grad) < 1e-5
        assert int(bad) == 0
    # out-of-range target: flagged, loss poisoned (ATen asserts on the device)
    tt = t.clone(); tt[1] = Cn
    xc, tc = x.cuda(), tt.cuda()
    L.check(lib.mnas_head_cross_entropy(xc.data_ptr(), tc.data_ptr(), N, Cn, -100, rows.data_ptr(),
                                        loss.data_ptr(), 0, bad.data_ptr(), L.cur_stream()))
    assert int(bad) == 1 and torch.isnan(loss).item()


# ---- per-element bounds (bounds_tail.head_gemm_interval / head_rowsum_interval / ce_intervals; tests/test_bounds_cpu.py proves on the
# CPU that they admit the kernels' arithmetic and reject the listed faults) ---------------------------------------------------------
def _at(t, offset=0):
    """t on the device as a view at element `offset` of a larger buffer (offset 1: a 4-byte, not 16-byte, aligned address)"""
    t = t.contiguous()
    buf = torch.full((t.numel() + 8,), float("nan"), dtype=t.dtype, device="cuda")
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _out(shape, init=None, offset=0):
    view, chk = G.guarded(shape, torch.float32, offset=offset)
    if init is not None:
        view.copy_(init)
    return view, chk


class _HeadCase:
    """one (N, I, O, p) with its inputs, the keep mask and the staged operand; off_*: element offsets of the device tensors"""

    def __init__(self, N, I, O_, p, scaled, off_in=0, off_out=0, off_x=None):
        self.N, self.I, self.O, self.p = N, I, O_, p
        self.seed = 0x1234567890ABCDEF ^ (N * 7919 + I)
        self.x, self.w, self.b, self.dz, self.u_prev, self.c0w, self.c0b = BT.head_inputs(N, I, O_, scaled)
        self.keep = _keep(self.seed, N, I, p)
        self.xd = BT.head_dropped(self.x, self.keep, p)
        self.post = self.keep.double() * BT.head_drop_scale(p) if p else None
        self.off_out = off_out
        self.xc = _at(self.x, off_in if off_x is None else off_x)
        self.wc, self.bc, self.dzc, self.uc = (_at(t, off_in) for t in (self.w, self.b, self.dz, self.u_prev))
        self.tag = "N %d I %d O %d p %g%s off %d/%d" % (N, I, O_, p, " scaled" if scaled else "", off_in, off_out)

    def args(self, relu=False, bias=True):
        return _lin(self.N, self.I, self.O, relu, self.p, self.seed, self.xc, self.wc, self.bc if bias else None)

    def fwd(self, relu, bias=True, A=None):
        y, chk = _out((self.N, self.O), offset=self.off_out)
        a = self.args(relu, bias)
        a.y = y.data_ptr()
        L.check(L.load().mnas_head_linear_fwd(Ct.byref(a), L.cur_stream()))
        chk(self.tag + " y")
        iv = BT.head_gemm_interval(self.xd if A is None else A, self.w.t(), self.b if bias else None, relu=relu)
        # (an output the ReLU clamps sits exactly on the lower end of its bracket, ratio 1: a family of its own)
        return IV.check_interval(y.cpu(), iv, "%s fwd relu %d bias %d" % (self.tag, relu, bias), "head gemm, ReLU" if relu else "head gemm"), iv

    def bwd_w(self, acc, B=None, dz=None):
        dw, cw = _out((self.O, self.I), self.c0w if acc else None, self.off_out)
        db, cb = _out((self.O,), self.c0b if acc else None, self.off_out)
        a = self.args()
        a.dz, a.dw, a.db, a.accumulate = self.dzc.data_ptr(), dw.data_ptr(), db.data_ptr(), acc
        L.check(L.load().mnas_head_linear_bwd_w(Ct.byref(a), L.cur_stream()))
        cw(self.tag + " dw")
        cb(self.tag + " db")
        dzt = (self.dz if dz is None else dz).t()
        iv = BT.head_gemm_interval(dzt, self.xd if B is None else B, C0=self.c0w if acc else None)
        r = IV.check_interval(dw.cpu(), iv, "%s dW acc %d" % (self.tag, acc), "head gemm")
        rb = IV.check_interval(db.cpu(), BT.head_rowsum_interval(dzt, self.c0b if acc else None), "%s db acc %d" % (self.tag, acc),
                              "head rowsum")
        return max(r, rb), iv

    def bwd_x(self, masked, dz=None):
        dx, chk = _out((self.N, self.I), offset=self.off_out)
        a = self.args()
        a.dz, a.dx = self.dzc.data_ptr(), dx.data_ptr()
        a.relu_mask = self.uc.data_ptr() if masked else None
        L.check(L.load().mnas_head_linear_bwd_x(Ct.byref(a), L.cur_stream()))
        chk(self.tag + " dx")
        mask = self.u_prev > 0 if masked else None
        iv = BT.head_gemm_interval(self.dz if dz is None else dz, self.w, post=self.post, mask=mask)
        got = dx.cpu()
        if masked:
            assert bool((got[~mask] == 0).all()), self.tag + ": dx not exactly 0 under a zero of the mask source"
            assert bool((self.u_prev == 0).any()) and (self.u_prev.numel() < 3 or bool((self.u_prev == 2.0 ** -149).any()))
        return IV.check_interval(got, iv, "%s dx masked %d" % (self.tag, masked), "head gemm"), iv

    def all(self):
        self.fwd(True)
        r = [self.fwd(False)[0], self.fwd(False, bias=False)[0], self.bwd_w(0)[0], self.bwd_w(1)[0],
             self.bwd_x(False)[0], self.bwd_x(True)[0]]
        return max(r)


@pytest.mark.parametrize("N,I,O_", BT.HEAD_SIZES)
@pytest.mark.parametrize("p", BT.HEAD_PS)
def test_linear_per_element_bound(N, I, O_, p):
    """EVERY element of y, dW, db, dx inside (L + 10) 2^-23 S of the fp64 result over the staged fp32 operands (derivation:
    bounds_tail.head_gemm_interval / head_rowsum_interval), plain inputs and inputs whose rows and columns are scaled by powers of
    two 2^-12 .. 2^12 (most outputs far below the tensor's maximum); bias NULL; dx exactly 0 where the
    mask source is +0.0 / -0.0 and not where it is the smallest subnormal; outputs inside canaries."""
    worst = max(_HeadCase(N, I, O_, p, scaled).all() for scaled in (False, True))
    print("head (%d, %d, %d) p %g: worst error / bound %.3f" % (N, I, O_, p, worst), IV.WORST)
    assert worst <= 1.0


@pytest.mark.parametrize("N,I,O_", [s for s in BT.HEAD_SIZES if s[1] % 4 == 0])
def test_linear_unaligned_operands(N, I, O_):
    """The sizes at which k_head_gemm<true> (16-byte loads) is eligible, with every operand and output at element offset 1 of
    its buffer (what Trainer's views of the flat parameter buffer look like behind a 10-class bias): k_head_gemm<false> on
    VEC-eligible shapes; then x alone unaligned; then everything aligned.  The same bound, canaries on both sides."""
    worst = 0.0
    for off_in, off_out, off_x in ((1, 1, None), (0, 0, 1), (0, 0, None)):
        c = _HeadCase(N, I, O_, 0.2, True, off_in, off_out, off_x)
        assert (c.xc.data_ptr() % 16 != 0) == ((off_in if off_x is None else off_x) == 1) and (c.wc.data_ptr() % 16 != 0) == (off_in == 1)
        worst = max(worst, c.all())
    print("head unaligned (%d, %d, %d): worst error / bound %.3f" % (N, I, O_, worst))


def test_linear_sparse_probe():
    """Live k = {0, 15, 16, 127, 128, K-1} only (both sides of a wave's 16-k slice and of the K step of 128), for all three
    entry points: S holds six terms, so one dropped, doubled or misplaced term leaves the bound -- each live term's contribution is
    asserted to exceed twice the bound at one of the probed rows {0, 31, 32, M-1} x columns {0, 31, 32, N-1}."""
    N, I, O_ = 130, 133, 131
    c = _HeadCase(N, I, O_, 0.0, False)
    x = BT.head_sparse(c.x, 1, I)
    c.xc = x.cuda()
    r, iv = c.fwd(False, A=x)
    BT.head_probe_visible(x, c.w.t(), iv, "fwd")
    c = _HeadCase(N, I, O_, 0.0, False)
    dz = BT.head_sparse(c.dz, 0, N)
    c.dzc = dz.cuda()
    r2, iv = c.bwd_w(0, dz=dz)
    BT.head_probe_visible(dz.t(), c.x, iv, "dW")
    dz = BT.head_sparse(c.dz, 1, O_)
    c.dzc = dz.cuda()
    r3, iv = c.bwd_x(False, dz=dz)
    BT.head_probe_visible(dz, c.w, iv, "dx")
    print("head sparse probes: error / bound %.3f %.3f %.3f" % (r, r2, r3))


def _ce_run(x, t, meters=None):
    N, Cn = x.shape
    rows, loss = torch.full((N,), 7.0, device="cuda"), torch.full((), 7.0, device="cuda")
    dl, chk = G.guarded((N, Cn), torch.float32)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    xc, tc = x.cuda(), t.cuda()
    L.check(L.load().mnas_head_cross_entropy(xc.data_ptr(), tc.data_ptr(), N, Cn, -100, rows.data_ptr(), loss.data_ptr(),
                                             dl.data_ptr(), bad.data_ptr(), L.cur_stream()))
    chk("cross-entropy dlogits")
    return dl.cpu(), rows.cpu(), loss.cpu(), int(bad)


@pytest.mark.parametrize("N,Cn", BT.CE_SIZES)
def test_cross_entropy_per_element_bracket(N, Cn):
    """EVERY dlogits element, every loss row and the mean inside the bracket bounds_tail.ce_intervals / ce_mean_interval propagate
    through k_head_ce's own roundings (expf, logf and the divisions at one ulp); N > 256 takes the count loop's and the mean's
    second trip; peaked rows, a common offset of +-1000 (logf(se) + mx - x[t] cancels), -inf logits, C = 1; ignored rows have
    exactly zero gradient; every row ignored: NaN loss, zero gradient."""
    worst = 0.0
    for kind in BT.CE_ROWS:
        x = BT.ce_logits(kind, N, Cn)
        for how in BT.CE_IGNORE:
            t = BT.ce_ignore(BT.ce_targets(N, Cn)[0], how)
            dl, rows, loss, bad = _ce_run(x, t)
            what = "ce %s / %s (%d, %d)" % (kind, how, N, Cn)
            iv = BT.ce_intervals(x, t)
            assert bad == 0 and iv["count"] == int((t != -100).sum()), what
            assert bool((dl[t == -100] == 0).all()) and bool((rows[t == -100] == 0).all()), what
            r = [IV.check_interval(dl, iv["dl"], what + " dlogits", "cross-entropy"), IV.check_interval(rows, iv["rows"], what + " rows", "cross-entropy"),
                 BT.check_ce_mean(loss, rows, iv["count"], what + " mean", "cross-entropy mean")]
            if how == "all":
                assert bool(torch.isnan(loss)) and bool((dl == 0).all()), what
            worst = max(worst, *r)
    if N > 1:                        # `bad` as before: a label out of range is flagged, poisons the loss, has no gradient
        x, t = BT.ce_logits("uniform4", N, Cn), BT.ce_targets(N, Cn)[0]
        t[N // 2] = Cn
        dl, rows, loss, bad = _ce_run(x, t)
        iv = BT.ce_intervals(x, t)
        ok = ~iv["nan_rows"]
        assert bad == 1 and bool(torch.isnan(loss)) and bool(torch.isnan(rows[N // 2])) and int(ok.sum()) == N - 1
        assert bool((dl[N // 2] == 0).all())
        IV.check_interval(dl, iv["dl"], "ce refused row, dlogits", "cross-entropy")
        IV.check_interval(rows[ok], IV.Interval(iv["rows"].lo[ok], iv["rows"].hi[ok]), "ce refused row, rows", "cross-entropy")
    print("cross-entropy (%d, %d): worst error / bracket %.3f" % (N, Cn, worst), {k: round(v, 4) for k, v in IV.WORST.items() if "entropy" in k})
    assert worst <= 1.0


def _classifier(cfg, num_classes=10):
    from mnasnet_pytorch_amd import FineTuneModelPool, load_model
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        m = FineTuneModelPool(load_model("mnasnet"), "mnasnet", num_classes, cfg)
    hst = O.init_head_state(cfg, num_classes, C.STATE_SEED)
    m.load_state_dict(hst, strict=False)
    return m.classifier.cuda(), hst


@pytest.mark.parametrize("cfg", C.HEADS)
@pytest.mark.parametrize("train", [False, True])
def test_head_module_matches_oracle(cfg, train):
    """NativeHead.apply (autograd path) on every classifier config: logits, input gradient and parameter gradients against the
    oracle run with the SAME keep masks (train) or without dropout (eval)."""
    seq, hst = _classifier(cfg)
    seq.train(train)
    head = NativeHead.build(seq)
    assert head is not None and len(head.layers) == sum(1 for l in O.HEAD_CONFIGS[cfg] if l[0] == "lin")
    N = 19
    f = (O.det_uniform((N, 320), 31).abs() * 2)
    fg = f.clone().cuda().requires_grad_(True)
    out = head.apply(fg)
    gl = O.det_uniform(tuple(out.shape), 32)
    out.backward(gl.cuda())
    keeps = None
    if train:
        seeds = [_mix(head.seed0, head.calls, i) for i in range(len(head.layers))]
        keeps = [_keep(s, N, l.lin.in_features, l.p) for s, l in zip(seeds, head.layers)]
        for i, l in enumerate(head.layers):      # the debug export agrees with what the GEMMs used
            assert torch.equal(head.dropout_mask(i, N, seeds[i]).cpu().bool(), keeps[i])
    fr = f.clone().double().requires_grad_(True)
    hd = {k: v.clone().double().requires_grad_(True) for k, v in hst.items()}
    ref = O.head_forward_masked(fr, hd, cfg, keeps)
    ref.backward(gl.double())
    assert relerr(out.detach().cpu(), ref.detach()) < TOL
    assert relerr(fg.grad.cpu(), fr.grad) < TOL
    for name, p in seq.named_parameters():
        assert relerr(p.grad.cpu(), hd["classifier." + name].grad) < TOL, name
    seq.zero_grad()


def test_native_step_matches_module_path():
    """Trainer.step without autograd (pool -> head -> cross-entropy -> backward as launch lists) against the same model
    stepped through model(x) / criterion / loss.backward(): identical kernels for the features, so loss, logits and every
    updated parameter agree to fp32 round-off of the head's gradient path."""
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_train import build, _no_dropout
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = torch.tensor([1, 3, 5, 7]).cuda()
    res = []
    for native in (True, False):
        m = build("512", proj_gamma=0.1).train(); _no_dropout(m)
        tr = Trainer(m, lr=1e-3)
        tr.native_step = native
        losses = [float(tr.step(x, t)) for _ in range(2)]
        res.append((losses, tr.flat_p.clone(), tr.last_logits))
        assert (tr._native_head() is not None) == native
    assert res[0][2] is not None and res[1][2] is None
    assert np.allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert relerr(res[0][1].cpu(), res[1][1].cpu()) < 1e-5


def test_native_step_dropout_runs_and_is_seeded():
    """with the reference's Dropout(0.5) active the step is reproducible under torch.manual_seed and differs across seeds"""
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_train import build
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = torch.tensor([1, 3, 5, 7]).cuda()
    out = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        m = build("512", proj_gamma=0.1).train()
        tr = Trainer(m, lr=1e-3)
        out.append([float(tr.step(x, t)) for _ in range(2)])
        assert all(np.isfinite(out[-1]))
    assert out[0] == out[1] and out[0] != out[2]
