"""-m gpu: the multi-label branch on the device (csrc/mnas_mlabel.hip, losses.py, metrics.MultiLabelMeters, Trainer.step / validate
with a MultiClassBCELoss) against tests/golden/multilabel.json (what the reference gave) and tests/multilabel_ref.py (the rule).

Bounds.  F1 and the integer counts: exact.  Dice: 4 * 2^-24 -- three fp32 roundings of magnitude <= 1 in 1 + log(2I/U) plus one for a
differing logf.  Loss and gradient: the bounds tests/test_gpu_head.py::test_cross_entropy holds the cross-entropy kernels to, against
an fp64 evaluation of the rule on the same inputs: |loss - ref| <= 2e-5 |ref| and max |dl - ref| < 1e-5 max |ref|."""
import json
import os

import numpy as np
import pytest
import torch

import cases as C
import multilabel_ref as R
from gpu_util import relerr
from mnasnet_pytorch_amd import HardDice, MultiClassBCELoss, MultiLabelMeters
from mnasnet_pytorch_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "multilabel.json")))
DICE_TOL = 4 * 2.0 ** -24
NAN = float("nan")
G = 64                                      # guard margin, elements (keeps 16-byte alignment)


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Bce:
    """one call of mnas_mlabel_bce into guarded buffers: NaN-filled margins around dlogits and the loss, 0xA5 bytes around the scratch;
    `ok()` checks that they are untouched.  misalign: the weights start 4 bytes past a 16-byte boundary."""

    def __init__(self, z, t, w=None, focal=False, gamma=R.FOCUS, balance=R.BALANCE, meters=None, nw=(0, 0, 0), grad=True, misalign=False):
        lib = L.load()
        N, Cn = z.shape
        self.N, self.Cn = N, Cn
        self.dl_buf = torch.full((N * Cn + 2 * G,), NAN, device="cuda")
        self.loss_buf = torch.full((2 * G + 1,), NAN, device="cuda")
        self.nb = int(lib.mnas_mlabel_scratch_bytes(N))
        self.scratch = torch.full((self.nb + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        wptr = 0
        if w is not None:
            off = 1 if misalign else 0
            self.wbuf = torch.zeros(N * Cn + 8, device="cuda")
            self.wbuf[off:off + N * Cn] = w.reshape(-1)
            wptr = self.wbuf.data_ptr() + 4 * off
            assert wptr % 16 == (4 if misalign else 0)
        self.grad = grad
        L.check(lib.mnas_mlabel_bce(z.data_ptr(), t.data_ptr(), wptr, N, Cn, 1 if focal else 0, float(gamma), float(balance),
                                    self.scratch.data_ptr() + G, self.loss_buf.data_ptr() + 4 * G,
                                    self.dl_buf.data_ptr() + 4 * G if grad else 0, meters.kernel_args(z.device) if meters else 0,
                                    nw[0], nw[1], nw[2], L.cur_stream()), "mlabel_bce")
        self.loss = self.loss_buf[G]
        self.dl = self.dl_buf[G:G + N * Cn].view(N, Cn)

    def ok(self):
        n = self.N * self.Cn
        assert bool(torch.isnan(self.dl_buf[:G]).all()) and bool(torch.isnan(self.dl_buf[G + n:]).all())
        assert bool(torch.isnan(self.loss_buf[:G]).all()) and bool(torch.isnan(self.loss_buf[G + 1:]).all())
        assert bool((self.scratch[:G] == 0xA5).all()) and bool((self.scratch[G + self.nb:] == 0xA5).all())
        if not self.grad:
            assert bool(torch.isnan(self.dl_buf).all())
        else:
            assert not bool(torch.isnan(self.dl).any()) or not bool(torch.isfinite(self.loss))
        return self


def _check_loss(call, z, t, w, focal, what):
    ref, g = R.bce(z.numpy(), t.numpy(), None if w is None else w.numpy(), focal)
    got = float(call.loss)
    err = abs(got - ref) / abs(ref)
    gerr = relerr(call.dl.cpu(), torch.from_numpy(g))
    assert err <= 2e-5, (what, got, ref, err)
    assert gerr < 1e-5, (what, gerr)
    return err, gerr


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", R.GRID_C)
def test_grid_metrics(C_):
    """every batch: F1 == the reference's, counts == the restatement's, Dice within the bound of the reference's; the fused entry, the
    metrics-only entry and the HardDice module agree bit for bit"""
    m_f, m_u = MultiLabelMeters(), MultiLabelMeters()
    hd, hd_d = HardDice(0.5), HardDice(0.5, deduct_intersection=True)
    worst = 0.0
    for (Cn, scale, density, seed) in [c for c in R.grid() if c[0] == C_]:
        key = R.grid_key(Cn, scale, density, seed)
        ref = GOLD["batches"][key]
        z, t, _ = R.grid_batch(Cn, scale, density, seed)
        zc, tc = z.cuda(), t.cuda()
        call = _Bce(zc, tc, meters=m_f, nw=(R.GRID_N,) * 3)
        m_u.update(zc, tc, call.loss)
        d0, d1 = hd(zc, tc), hd_d(zc, tc)
        assert d0.dtype == torch.float32 and d0.dim() == 0 and d0.is_cuda
        torch.cuda.synchronize()
        call.ok()
        assert torch.equal(m_f.block, m_u.block), key
        rec = m_f.read()
        assert rec.f1.val == ref["f1"], (key, rec.f1.val, ref["f1"])
        assert (rec.last_tp, rec.last_fp, rec.last_fn) == R.dice_counts(z.numpy(), t.numpy()), key
        assert rec.hdice.val == float(d0), key                                        # meters and module: the same bits
        worst = max(worst, abs(rec.hdice.val - ref["hdice"]["False"]), abs(float(d1) - ref["hdice"]["True"]))
        assert abs(rec.hdice.val - ref["hdice"]["False"]) <= DICE_TOL, (key, rec.hdice.val, ref["hdice"])
        assert abs(float(d1) - ref["hdice"]["True"]) <= DICE_TOL, (key, float(d1), ref["hdice"])
        assert rec.loss.val == float(call.loss) and rec.last_n == R.GRID_N
    rec = m_f.read()
    assert rec.steps == 30 and rec.samples == 30 * R.GRID_N == rec.loss_n == rec.hdice_n == rec.f1_n and rec.nonfinite_steps == 0
    print("C %d: largest Dice difference to the reference %.3g (bound %.3g)" % (C_, worst, DICE_TOL))


@pytest.mark.parametrize("C_", R.GRID_C)
def test_grid_loss_and_gradient(C_):
    """all four variants against the fp64 rule; the fused-with-meters entry gives bitwise the loss and gradient of the plain one"""
    m = MultiLabelMeters()
    worst = [0.0, 0.0]
    for (Cn, scale, density, seed) in [c for c in R.grid() if c[0] == C_]:
        z, t, w = R.grid_batch(Cn, scale, density, seed)
        zc, tc, wc = z.cuda(), t.cuda(), w.cuda()
        for name, weighted, focal in R.LOSS_VARIANTS:
            a = _Bce(zc, tc, wc if weighted else None, focal)
            b = _Bce(zc, tc, wc if weighted else None, focal, meters=m, nw=(R.GRID_N,) * 3)
            torch.cuda.synchronize()
            a.ok(), b.ok()
            assert torch.equal(_bits(a.loss), _bits(b.loss)) and torch.equal(_bits(a.dl), _bits(b.dl)), (name, Cn, scale, seed)
            e, ge = _check_loss(a, z, t, w if weighted else None, focal, (name, Cn, scale, density, seed))
            worst = [max(worst[0], e), max(worst[1], ge)]
    print("C %d: largest loss error %.3g (bound 2e-5), gradient %.3g (bound 1e-5)" % (C_, worst[0], worst[1]))


def test_module_forward_backward():
    """MultiClassBCELoss as an nn.Module: the loss of the raw entry, d loss / d outputs = dlogits * grad_output, weights ignored
    unless use_weight_mask; forward only without requires_grad"""
    z, t, w = R.grid_batch(90, 2.0, 0.3, 1)
    zc, tc, wc = z.cuda(), t.cuda(), w.cuda()
    for name, weighted, focal in R.LOSS_VARIANTS:
        raw = _Bce(zc, tc, wc if weighted else None, focal)
        crit = MultiClassBCELoss(use_weight_mask=weighted, use_focal_weights=focal)
        zr = zc.clone().requires_grad_(True)
        loss = crit(zr, tc, wc)
        (loss * 3.0).backward()
        assert torch.equal(_bits(loss.detach()), _bits(raw.loss)), name
        assert torch.equal(_bits(zr.grad), _bits(raw.dl * 3.0)), name
        with torch.no_grad():
            assert torch.equal(_bits(crit(zc, tc, wc)), _bits(raw.loss))
    # int targets are converted with .float(); the focal parameters reach the kernel
    crit = MultiClassBCELoss(use_focal_weights=True, focus_param=3, balance_param=0.5)
    got = float(crit(zc, tc.long()))
    ref = R.bce(z.numpy(), t.numpy(), None, True, 3, 0.5)[0]
    assert abs(got - ref) <= 2e-5 * abs(ref)


# ---- shapes where the kernel can go wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cn", [(1, 1), (3, 5), (7, 63), (7, 65), (5, 257), (2, 1000), (257, 3)])
def test_shapes(N, Cn):
    """one class; a partial wave; just under / over one wave; one past the workgroup's stride with C % 4 != 0; the 16-byte path; N
    past the batch stage's stride.  Guarded outputs, weights 4 bytes off 16-byte alignment (the scalar path), aligned (the vector
    path where C % 4 == 0), forward only."""
    g = torch.Generator().manual_seed(N * 1000 + Cn)
    t = (torch.rand(N, Cn, generator=g) < 0.4).float()
    z = (torch.randn(N, Cn, generator=g) + 0.5 * (2 * t - 1)) * 2.0
    w = 0.25 + 1.5 * torch.rand(N, Cn, generator=g)
    zc, tc, wc = z.cuda(), t.cuda(), w.cuda()
    f1, counts = R.f1_batch(z.numpy(), t.numpy()), R.dice_counts(z.numpy(), t.numpy())
    dice = R.hard_dice(z.numpy(), t.numpy())
    for name, weighted, focal in R.LOSS_VARIANTS:
        for misalign in ((False, True) if weighted else (False,)):
            m = MultiLabelMeters()
            call = _Bce(zc, tc, wc if weighted else None, focal, meters=m, nw=(N, N, 3), misalign=misalign)
            fwd = _Bce(zc, tc, wc if weighted else None, focal, grad=False, misalign=misalign)
            torch.cuda.synchronize()
            call.ok(), fwd.ok()
            _check_loss(call, z, t, w if weighted else None, focal, (name, misalign))
            assert torch.equal(_bits(fwd.loss), _bits(call.loss))
            rec = m.read()
            assert rec.f1.val == f1 and (rec.last_tp, rec.last_fp, rec.last_fn) == counts and abs(rec.hdice.val - dice) <= DICE_TOL
            assert (rec.steps, rec.samples, rec.loss_n, rec.hdice_n, rec.f1_n) == (1, N, N, N, 3)
    m = MultiLabelMeters()
    m.update(zc, tc, f1_n=3)
    rec = m.read()
    assert rec.f1.val == f1 and (rec.tp, rec.fp, rec.fn) == counts and rec.loss_n == 0 and rec.f1_n == 3
    assert abs(float(HardDice()(zc, tc)) - dice) <= DICE_TOL
    th = 0.7                                                 # another threshold: predicted iff z > logit(0.7)
    assert abs(float(HardDice(th, True)(zc, tc)) - R.hard_dice(z.numpy(), t.numpy(), np.log(th / (1 - th)), True)) <= DICE_TOL


# ---- edge rows --------------------------------------------------------------------------------------------------------------------------
def test_edge_rows():
    # exact-zero logits: positive for F1, negative for Dice
    z = torch.zeros(2, 4)
    t = torch.tensor([[1.0, 0, 0, 1], [0, 0, 0, 0]])
    m = MultiLabelMeters()
    call = _Bce(z.cuda(), t.cuda(), meters=m, nw=(2, 2, 2)).ok()
    rec = m.read()
    assert rec.f1.val == R.f1_batch(z.numpy(), t.numpy()) == ((4 / 6 + 0.0) / 2 + 0.0) / 2
    assert (rec.tp, rec.fp, rec.fn) == (0, 0, 2) and rec.hdice.val == 0.0
    assert abs(float(call.loss) - np.log(2.0)) <= 2e-5 * np.log(2.0)
    one = torch.tensor([[0.0]])
    m.reset()
    m.update(one.cuda(), torch.ones(1, 1).cuda())
    rec = m.read()
    assert rec.f1.val == 1.0 and rec.hdice.val == 0.0 and (rec.tp, rec.fp, rec.fn) == (0, 0, 1)
    # everything right / everything wrong / nothing there
    t = torch.tensor([[1.0, 0, 1, 0]])
    for z, want in ((torch.tensor([[3.0, -3, 2, -1]]), (1.0, 1.0)), (torch.tensor([[-3.0, 3, -2, 1]]), (0.0, 0.0))):
        m.reset()
        m.update(z.cuda(), t.cuda())
        rec = m.read()
        assert (rec.f1.val, rec.hdice.val) == want
    m.reset()
    m.update(torch.tensor([[-1.0, -2, -0.5]]).cuda(), torch.zeros(1, 3).cuda())
    rec = m.read()
    assert (rec.f1.val, rec.hdice.val) == (1.0, 0.0)
    # NaN and Inf logits: a non-finite loss, counted once; the NaN is predicted negative under both rules
    z = torch.tensor([[NAN, 1.0, 1.0, -2.0], [1.0, float("inf"), -1.0, -1.0], [0.5, -0.5, float("-inf"), 2.0]])
    t = torch.tensor([[1.0, 0, 1, 0], [1.0, 1, 0, 0], [0.0, 0, 1, 1]])
    m.reset()
    bad = _Bce(z.cuda(), t.cuda(), meters=m, nw=(3, 3, 3)).ok()
    fine = _Bce(torch.nan_to_num(z, 0.0, 9.0, -9.0).cuda(), t.cuda(), meters=m, nw=(3, 3, 3)).ok()
    rec = m.read()
    assert not np.isfinite(float(bad.loss)) and np.isfinite(float(fine.loss))
    assert rec.nonfinite_steps == 1 and rec.steps == 2
    m.reset()
    m.update(z.cuda(), t.cuda())
    rec = m.read()
    assert (rec.tp, rec.fp, rec.fn) == R.dice_counts(z.numpy(), t.numpy()) == (4, 2, 2)
    assert rec.f1.val == R.f1_batch(z.numpy(), t.numpy()) and abs(rec.hdice.val - R.hard_dice(z.numpy(), t.numpy())) <= DICE_TOL
    # soft targets enter the loss and are negatives for the metrics
    z, t, w = R.grid_batch(90, 2.0, 0.3, 2)
    t = torch.where(torch.rand(t.shape, generator=torch.Generator().manual_seed(5)) < 0.3, torch.full_like(t, 0.3), t)
    m.reset()
    call = _Bce(z.cuda(), t.cuda(), w.cuda(), True, meters=m, nw=(12, 12, 12)).ok()
    _check_loss(call, z, t, w, True, "soft targets")
    rec = m.read()
    assert (rec.tp, rec.fp, rec.fn) == R.dice_counts(z.numpy(), t.numpy()) and rec.f1.val == R.f1_batch(z.numpy(), t.numpy())
    assert rec.tp + rec.fn == int((t == 1).sum())


# ---- meters ------------------------------------------------------------------------------------------------------------------------------
def test_meters_are_the_host_average_meters():
    """ten updates with unequal N and f1_n = 3: val / avg / sum / count of all three meters equal host AverageMeters fed with the
    device's own per-batch values, to the bit; fused entry and update() hold identical blocks; reset() zeroes the block"""
    sizes = [12, 7, 256, 1, 33, 12, 100, 5, 64, 300]
    m_f, m_u = MultiLabelMeters(), MultiLabelMeters()
    log = R.StepLog()
    for i, N in enumerate(sizes):
        g = torch.Generator().manual_seed(700 + i)
        t = (torch.rand(N, 90, generator=g) < 0.2).float()
        z = (torch.randn(N, 90, generator=g) + 0.8 * (2 * t - 1)) * (0.5 + i)
        zc, tc = z.cuda(), t.cuda()
        call = _Bce(zc, tc, meters=m_f, nw=(N, N, 3))
        m_u.update(zc, tc, call.loss, f1_n=3)
        rec = m_f.read()
        assert rec.f1.val == R.f1_batch(z.numpy(), t.numpy()) and rec.loss.val == float(call.loss)
        log.update(z.numpy(), t.numpy(), rec.loss.val, rec.hdice.val, rec.f1.val, N, N, 3)
        log.check(rec)
        log.check(m_u.read())
    rec = m_f.read()
    assert rec.steps == 10 and rec.samples == sum(sizes) == rec.loss_n == rec.hdice_n and rec.f1_n == 30
    assert torch.equal(m_f.block, m_u.block)
    print(rec)
    m_f.reset()
    assert not bool(m_f.block.any()) and m_f.read().steps == 0 and m_f.read().f1.avg == 0.0


def test_update_is_capturable_in_a_graph():
    """a linear single-stream capture of one update() and one fused loss call: three replays move the block three times each"""
    z, t, _ = R.grid_batch(1000, 2.0, 0.3, 0)
    zc, tc = z.cuda(), t.cuda()
    m = MultiLabelMeters()
    crit = MultiClassBCELoss(use_focal_weights=True)
    from mnasnet_pytorch_amd.losses import bce_with_logits
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.update(zc, tc)
        bce_with_logits(zc, tc, None, True, crit.focus_param, crit.balance_param, meters=m, meter_weights=(12, 12, 3))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        m.update(zc, tc)
        loss, dl = bce_with_logits(zc, tc, None, True, crit.focus_param, crit.balance_param, meters=m, meter_weights=(12, 12, 3))
    for _ in range(3):
        graph.replay()
    rec = m.read()
    ref = GOLD["batches"][R.grid_key(1000, 2.0, 0.3, 0)]
    assert rec.steps == 6 and rec.samples == 72 and rec.loss_n == 36 and rec.f1_n == 3 * 12 + 3 * 3
    assert rec.f1.val == ref["f1"] and abs(float(loss) - ref["loss64"]["focal"]) <= 2e-5 * ref["loss64"]["focal"]
    tp, fp, fn = R.dice_counts(z.numpy(), t.numpy())
    assert (rec.tp, rec.fp, rec.fn) == (6 * tp, 6 * fp, 6 * fn)


# ---- step ----------------------------------------------------------------------------------------------------------------------------------
def _ml_target(N, classes=10, shift=0):
    return (((torch.arange(N)[:, None] * 3 + torch.arange(classes)[None, :] + shift) % 4) == 0).float()


def _trainer(meters, native, crit=None):
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_train import _no_dropout, build
    torch.manual_seed(11)
    m = build("512", proj_gamma=0.1).train()
    _no_dropout(m)
    tr = Trainer(m, lr=1e-3, criterion=crit if crit is not None else MultiClassBCELoss(), meters=meters)
    tr.native_step = native
    return m, tr


def test_trainer_step_native_bce():
    """FineTuneModelPool, head '512', 10 classes, 4 x 3 x 64 x 64 (the model test_trainer_matches_torch_optimizer_path builds): the
    native BCE step against its native_step = False twin within that test's bounds; the fp64 rule on last_logits reproduces the
    step's loss and the last Linear's bias gradient; meters change no bit of the loss; the meters' weights are N, N and
    input.size(1)"""
    x = C.det_input((4, 3, 64, 64)).cuda()
    target = _ml_target(4).cuda()
    runs = {}
    for name, meters, native in (("native+meters", True, True), ("native", False, True), ("module+meters", True, False)):
        mm = MultiLabelMeters() if meters else None
        m, tr = _trainer(mm, native)
        assert (tr._native_head() is not None) == native
        losses, extra = [], None
        for i in range(3):
            loss = tr.step(x, target)
            assert loss.grad_fn is None and not loss.requires_grad
            if native:
                assert tr.last_logits is not None and tr.last_logits.shape == (4, 10)      # the native path was taken
            else:
                assert tr.last_logits is None
            if i == 0 and native:
                lin = [mod for mod in m.classifier if isinstance(mod, torch.nn.Linear)][-1]
                extra = (tr.last_logits.cpu().clone(), lin.bias.grad.cpu().clone())
            losses.append(loss.clone())
        torch.cuda.synchronize()
        runs[name] = (losses, extra, mm.read() if mm else None, tr.last_logits)
    l1, l2 = [float(v) for v in runs["module+meters"][0]], [float(v) for v in runs["native"][0]]
    print("module path", l1, "native", l2)
    assert abs(l1[0] - l2[0]) <= 5e-3 * abs(l1[0]), (l1, l2)
    assert abs(l1[2] - l2[2]) <= 3e-2 * abs(l1[2]), (l1, l2)
    assert torch.equal(_bits(runs["native+meters"][0][0]), _bits(runs["native"][0][0]))          # first step: the same loss bits
    logits, bgrad = runs["native"][1]
    ref, g = R.bce(logits.numpy(), target.cpu().numpy())
    assert abs(l2[0] - ref) <= 2e-5 * abs(ref), (l2[0], ref)
    assert relerr(bgrad, torch.from_numpy(g.sum(0))) < 1e-5
    for name in ("native+meters", "module+meters"):
        rec = runs[name][2]
        assert (rec.steps, rec.samples, rec.loss_n, rec.hdice_n, rec.f1_n, rec.nonfinite_steps) == (3, 12, 12, 12, 9, 0), name
        assert rec.loss.val == float(runs[name][0][2])
    rec, last = runs["native+meters"][2], runs["native+meters"][3].cpu().numpy()
    assert rec.f1.val == R.f1_batch(last, target.cpu().numpy())
    assert (rec.last_tp, rec.last_fp, rec.last_fn) == R.dice_counts(last, target.cpu().numpy())
    # the focal / weighted settings of the criterion reach the step; a shape mismatch is refused
    m, tr = _trainer(None, True, MultiClassBCELoss(use_focal_weights=True))
    lf = float(tr.step(x, target))
    ref = R.bce(tr.last_logits.cpu().numpy(), target.cpu().numpy(), None, True)[0]
    assert abs(lf - ref) <= 2e-5 * abs(ref)
    with pytest.raises(ValueError):
        tr.step(x, target[:, :5])
    with pytest.raises(ValueError):
        tr.step(x, torch.tensor([1, 3, 5, 7]).cuda())
    # meters of the wrong kind are refused by the constructor, and on either path before a gradient is formed
    from mnasnet_pytorch_amd import DeviceMeters
    from mnasnet_pytorch_amd.train_step import Trainer
    with pytest.raises(ValueError):
        Trainer(m, lr=1e-3, criterion=MultiClassBCELoss(), meters=DeviceMeters((1,)))
    tr.meters = DeviceMeters((1,))
    for native in (True, False):
        tr.native_step = native
        with pytest.raises(ValueError):
            tr.step(x, target)
        assert not bool(tr.flat_g.any())                    # step() had zeroed it; nothing was accumulated
    # a subclass may override forward(): it keeps the module path, and what it computes is what the step returns
    class Doubled(MultiClassBCELoss):
        def forward(self, outputs, targets, weights=None):
            return super().forward(outputs, targets, weights) * 2

    tr.native_step, tr.meters, tr.criterion = True, None, Doubled()
    assert tr._native_head() is None
    seen = []
    hook = m.register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))
    l2x = float(tr.step(x, target))
    hook.remove()
    ref = 2 * R.bce(seen[-1].cpu().numpy(), target.cpu().numpy())[0]
    assert abs(l2x - ref) <= 2e-5 * abs(ref), (l2x, ref)


# ---- validate ----------------------------------------------------------------------------------------------------------------------------
def test_validate_multilabel_equals_hand_loop_with_one_sync(monkeypatch):
    from mnasnet_pytorch_amd import DeviceMeters
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_train import build
    torch.manual_seed(3)
    m = build("512", proj_gamma=0.1).train()               # dropout stays at 0.5: eval mode must switch it off
    with pytest.raises(ValueError):
        Trainer(m, lr=1e-3, meters=MultiLabelMeters())      # a cross-entropy criterion (the default) with multi-label meters
    tr = Trainer(m, lr=1e-3, criterion=MultiClassBCELoss())
    tr.step(C.det_input((8, 3, 96, 128)).cuda(), _ml_target(8).cuda())     # running statistics away from their init
    shapes = [(96, 128), (128, 96), (96, 128)]
    batches = [(C.det_input((8, 3) + shapes[i], seed=C.INPUT_SEED + 40 + i).cuda(), _ml_target(8, shift=i).cuda()) for i in range(3)]
    # train.py:556-587 by hand: model.eval(), no_grad, model(x), the rule in fp64, the restatement; weights N, N, input.size(1)
    log = R.StepLog()
    m.eval()
    with torch.no_grad():
        for x, t in batches:
            out, tt = m(x).cpu().numpy(), t.cpu().numpy()
            log.update(out, tt, R.bce(out, tt)[0], R.hard_dice(out, tt), R.f1_batch(out, tt), 8, 8, 3)
    m.train()
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    tr.validate(batches)                                    # programs of both shapes exist from here on
    count = {"n": 0, "in_read": False}
    real_read = MultiLabelMeters.read

    def read(self):
        count["in_read"] = True
        try:
            return real_read(self)
        finally:
            count["in_read"] = False

    def counting(fn):
        def wrapped(*a, **k):
            if not count["in_read"]:
                count["n"] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(MultiLabelMeters, "read", read)
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counting(getattr(torch.Tensor, name)))
    monkeypatch.setattr(torch.cuda, "synchronize", counting(torch.cuda.synchronize))
    try:
        rec = tr.validate(batches)
    finally:
        monkeypatch.undo()
    assert count["n"] == 0, "validate() took %d synchronising calls before read()" % count["n"]
    print("validate:", rec, "| hand loop", log.loss.state(), log.hdice.state(), log.f1.state())
    assert (rec.steps, rec.samples, rec.loss_n, rec.hdice_n, rec.f1_n, rec.nonfinite_steps) == (3, 24, 24, 24, 9, 0)
    assert (rec.tp, rec.fp, rec.fn) == (log.tp, log.fp, log.fn) and (rec.last_tp, rec.last_fp, rec.last_fn) == log.last
    assert rec.f1.avg == log.f1.avg and rec.f1.val == log.f1.val
    assert abs(rec.hdice.avg - log.hdice.avg) <= DICE_TOL and abs(rec.hdice.val - log.hdice.val) <= DICE_TOL
    assert abs(rec.loss.avg - log.loss.avg) <= 2e-5 * abs(log.loss.avg) and abs(rec.loss.val - log.loss.val) <= 2e-5 * abs(log.loss.val)
    assert m.training and all(mod.training for mod in m.modules())
    for k, v in m.named_buffers():
        assert torch.equal(v, bufs[k]), k
    # a caller's meters accumulate; the wrong kind of meters is refused either way round
    mine = MultiLabelMeters()
    tr.validate(batches, meters=mine, max_batches=2)
    assert tr.validate(batches, meters=mine).steps == 5
    with pytest.raises(ValueError):
        tr.validate(batches, meters=DeviceMeters((1, 5)))
    tr.criterion = torch.nn.CrossEntropyLoss()
    try:
        with pytest.raises(ValueError):
            tr.validate(batches, meters=MultiLabelMeters())
    finally:
        tr.criterion = MultiClassBCELoss()
    assert m.training and all(mod.training for mod in m.modules())
    # the module path (native_step = False) feeds the same meters through the metrics-only entry
    tr.native_step = False
    rec2 = tr.validate(batches)
    assert (rec2.tp, rec2.fp, rec2.fn, rec2.f1_n) == (rec.tp, rec.fp, rec.fn, 9) and rec2.f1.avg == rec.f1.avg
    assert abs(rec2.loss.avg - rec.loss.avg) <= 2e-5 * abs(rec.loss.avg)
