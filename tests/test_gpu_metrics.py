"""-m gpu: the device-resident loss / top-k accuracy meters (csrc/mnas_head.hip "MnasMeters", mnasnet_pytorch_amd/metrics.py,
Trainer(meters=...), Trainer.validate) -- train.py:447,465-468,556-592,657-700 without the three host reads per batch.

Kernel level: both entry points give, on every batch of the fixture's grid, exactly the counts the reference's accuracy() recorded
(tests/golden/metrics.json); ties, ignored / out-of-range / NaN rows and k > C follow the rule stated in include/mnas.h; the fused
entry's loss, dlogits and bad flag are BITWISE those of mnas_head_cross_entropy; the loss meter is bit for bit a host AverageMeter
fed with loss.item().  Step level: a trainer with meters and its twin without end up with the same bits.  validate(): one host sync.
Nothing here reads the reference: the fixture and tests/metrics_ref.py (the independent restatement) are the yardsticks."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases as C
import metrics_ref as R
from mnasnet_pytorch_amd import _lib as L
from mnasnet_pytorch_amd.metrics import DeviceMeters, accuracy

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(C.GOLDEN_DIR, "metrics.json")))


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class _Loss:
    """the raw mnas_head_cross_entropy[_metrics] call with its own scratch"""

    def __init__(self, N, Cn):
        self.N, self.Cn = N, Cn
        self.rows = torch.empty(N, device="cuda")
        self.loss = torch.full((), float("nan"), device="cuda")
        self.dl = torch.full((N, Cn), float("nan"), device="cuda")
        self.bad = torch.zeros(1, dtype=torch.int32, device="cuda")

    def plain(self, z, t, ignore=-100):
        L.check(L.load().mnas_head_cross_entropy(z.data_ptr(), t.data_ptr(), self.N, self.Cn, ignore, self.rows.data_ptr(),
                                                 self.loss.data_ptr(), self.dl.data_ptr(), self.bad.data_ptr(), L.cur_stream()))
        return self

    def fused(self, z, t, meters, ignore=-100):
        ks, nk, ranks, blk = meters.kernel_args(self.N, z.device)
        L.check(L.load().mnas_head_cross_entropy_metrics(z.data_ptr(), t.data_ptr(), self.N, self.Cn, ignore, self.rows.data_ptr(),
                                                         self.loss.data_ptr(), self.dl.data_ptr(), self.bad.data_ptr(), ks, nk, ranks,
                                                         blk, L.cur_stream()))
        return self


@pytest.mark.parametrize("Cn", R.GRID_C)
@pytest.mark.parametrize("scale", R.GRID_SCALE)
def test_grid_counts_equal_reference(Cn, scale):
    """every batch of the grid, both entry points and accuracy(): exactly the reference's prec@1 / prec@5"""
    m_plain, m_fused = DeviceMeters((1, 5)), DeviceMeters((1, 5))
    ce = _Loss(R.GRID_N, Cn)
    want1 = want5 = 0
    for seed in R.GRID_SEEDS:
        z, t = R.grid_batch(Cn, scale, seed)
        ref = GOLD["batches"][R.grid_key(Cn, scale, seed)]
        zc, tc = z.cuda(), t.cuda()
        m_plain.update(zc, tc)
        ce.fused(zc, tc, m_fused)
        a1, a5 = accuracy(zc, tc, topk=(1, 5))
        assert a1.is_cuda and a1.dim() == 0 and a1.dtype == torch.float32
        ra, rb = m_plain.read(), m_fused.read()
        print("C %d scale %g seed %d: prec1 %.4f prec5 %.4f (reference %.4f %.4f)" % (Cn, scale, seed, ra.acc[1].val, ra.acc[5].val,
                                                                                       ref["prec1"], ref["prec5"]))
        for got in ((ra.acc[1].val, ra.acc[5].val), (rb.acc[1].val, rb.acc[5].val), (float(a1), float(a5))):
            assert got == (ref["prec1"], ref["prec5"]) == (ref["prec1_softmax"], ref["prec5_softmax"]), (Cn, scale, seed)
        want1 += round(ref["prec1"] * R.GRID_N / 100)
        want5 += round(ref["prec5"] * R.GRID_N / 100)
    for rec in (m_plain.read(), m_fused.read()):
        assert (rec.correct[1], rec.correct[5], rec.samples, rec.steps) == (want1, want5, 10 * R.GRID_N, 10)
    assert m_plain.read().loss_samples == 0 and m_fused.read().loss_samples == 10 * R.GRID_N


def test_ties_go_to_the_lower_index():
    """equal logits before and after the target index: rank = #greater + #equal at a LOWER index (our rule; torch.topk's order of
    equal values is unspecified, so this is not compared with torch)"""
    row = [1.0, 2.0, 2.0, 2.0, 0.0, 2.0, 2.0, 2.0, 2.0, 2.0]
    z = torch.tensor([row] * 6).cuda()
    t = torch.tensor([1, 3, 6, 7, 0, 4]).cuda()           # ranks 0, 2, 4, 5, 8, 9
    assert R.ranks(z.cpu().numpy(), t.cpu().numpy()).tolist() == [0, 2, 4, 5, 8, 9]
    for fused in (False, True):
        m = DeviceMeters((1, 5, 3, 7))
        if fused:
            _Loss(6, 10).fused(z, t, m)
        else:
            m.update(z, t)
        rec = m.read()
        assert rec.last_correct == {1: 1, 5: 3, 3: 2, 7: 4} == rec.correct and rec.samples == 6


def test_bad_rows_count_as_wrong():
    """ignore_index, out-of-range and NaN-target rows are wrong for every k and still count in samples; an out-of-range target sets the
    existing bad flag and poisons the loss (nonfinite_steps), an ignored row does neither"""
    g = torch.Generator().manual_seed(5)
    z = torch.randn(8, 10, generator=g)
    t = z.argmax(1)                                       # every row right at k = 1 ...
    zc = z.cuda()
    # (a) ignored rows
    ta = t.clone(); ta[[1, 4]] = -100
    m = DeviceMeters((1, 5)); ce = _Loss(8, 10).fused(zc, ta.cuda(), m)
    rec = m.read()
    assert rec.last_correct == {1: 6, 5: 6} and rec.samples == 8 and int(ce.bad) == 0 and rec.nonfinite_steps == 0
    assert rec.loss.val == float(ce.loss) and np.isfinite(rec.loss.val)
    # (b) out of range: flagged, loss NaN, step counted as non-finite
    tb = t.clone(); tb[2] = 10; tb[5] = -1
    m = DeviceMeters((1, 5)); ce = _Loss(8, 10).fused(zc, tb.cuda(), m)
    rec = m.read()
    assert rec.last_correct == {1: 6, 5: 6} and rec.samples == 8 and int(ce.bad) == 1
    assert rec.nonfinite_steps == 1 and np.isnan(rec.loss.val) and np.isnan(rec.loss_sum)
    m2 = DeviceMeters((1, 5)); m2.update(zc, tb.cuda()); m2.update(zc, ta.cuda())      # no ignore_index there: -100 is out of range
    assert m2.read().correct == {1: 12, 5: 12} and m2.read().samples == 16
    # (c) NaN / Inf target logit: wrong; NaN elsewhere in the row: comparisons with NaN are false
    zn = z.clone(); zn[0, t[0]] = float("nan"); zn[3, t[3]] = float("inf"); zn[6, (int(t[6]) + 1) % 10] = float("nan")
    m = DeviceMeters((1, 5)); ce = _Loss(8, 10).fused(zn.cuda(), t.cuda(), m)
    rec = m.read()
    assert rec.last_correct == {1: 6, 5: 6} and rec.nonfinite_steps == 1 and int(ce.bad) == 0
    m2 = DeviceMeters((1, 5)); m2.update(zn.cuda(), t.cuda(), torch.tensor(1.5).cuda())
    rec = m2.read()
    assert rec.last_correct == {1: 6, 5: 6} and rec.nonfinite_steps == 0 and rec.loss.val == 1.5 and rec.loss_sum == 12.0
    assert R.correct_counts(zn.numpy(), t.numpy(), (1, 5)) == {1: 6, 5: 6}


@pytest.mark.parametrize("N", [1, 7, 256])
@pytest.mark.parametrize("Cn", [2, 10, 1000, 5000])
def test_shapes_and_fused_entry_is_bitwise_the_plain_loss(N, Cn):
    """N x C corners, k > C clamped to C; loss, dlogits and flag of the fused entry == mnas_head_cross_entropy bit for bit, also with
    ignored and out-of-range rows in the batch"""
    g = torch.Generator().manual_seed(N * 10007 + Cn)
    z = torch.randn(N, Cn, generator=g) * 3
    t = torch.randint(0, Cn, (N,), generator=g)
    z[torch.arange(0, N, 2), t[::2]] += 6.0
    for variant in ("clean", "ignored", "out_of_range"):
        tt = t.clone()
        if variant == "ignored":
            tt[::3] = -100
        if variant == "out_of_range":
            tt[N // 2] = Cn
        zc, tc = z.cuda(), tt.cuda()
        m_f, m_p = DeviceMeters((1, 5, 6000)), DeviceMeters((1, 5, 6000))
        a = _Loss(N, Cn).plain(zc, tc)
        b = _Loss(N, Cn).fused(zc, tc, m_f)
        m_p.update(zc, tc)
        assert torch.equal(_bits(a.loss), _bits(b.loss)) and torch.equal(_bits(a.dl), _bits(b.dl)) and torch.equal(a.bad, b.bad)
        assert torch.equal(_bits(a.rows), _bits(b.rows))
        want = R.correct_counts(z.numpy(), tt.numpy(), (1, 5, 6000), ignore_index=-100)
        rec = m_f.read()
        assert rec.last_correct == want and rec.samples == N and rec.last_n == N, (variant, rec.last_correct, want)
        assert m_p.read().last_correct == R.correct_counts(z.numpy(), tt.numpy(), (1, 5, 6000))
        if variant == "clean":
            assert want[6000] == N and (Cn > 5 or want[5] == N)            # k >= C: every valid row is correct
            assert rec.loss.val == float(b.loss) and rec.loss_sum == float(b.loss) * N


def test_loss_meter_is_the_host_average_meter():
    """ten updates with different batch sizes: loss_sum, samples, val, avg equal a host AverageMeter fed with the ten loss.item()
    values exactly (double arithmetic in the same order); through the fused entry and through update(loss=...); two runs give
    identical blocks"""
    sizes = [256, 256, 100, 7, 256, 33, 1, 256, 64, 100]
    blocks = []
    for run in range(2):
        m_f, m_u = DeviceMeters((1, 5)), DeviceMeters((1, 5))
        log = R.StepLog((1, 5))
        for i, N in enumerate(sizes):
            g = torch.Generator().manual_seed(900 + i)
            z = torch.randn(N, 1000, generator=g) * (0.5 + i)
            t = torch.randint(0, 1000, (N,), generator=g)
            z[torch.arange(0, N, 2), t[::2]] += 2.0 * (0.5 + i)
            zc, tc = z.cuda(), t.cuda()
            ce = _Loss(N, 1000).fused(zc, tc, m_f)
            m_u.update(zc, tc, ce.loss)
            log.update(z.numpy(), t.numpy(), ce.loss.item())
            if i in (0, 4, 9):
                log.check(m_f.read())
                log.check(m_u.read())
        rec = m_f.read()
        assert rec.steps == 10 and rec.samples == sum(sizes) == rec.loss_samples
        assert rec.loss_sum == log.loss.sum and rec.loss.avg == log.loss.avg and rec.loss.val == log.loss.val
        print("run %d: %r" % (run, rec))
        torch.cuda.synchronize()
        assert torch.equal(m_f.block, m_u.block)
        blocks.append(m_f.block.clone())
        m_f.reset()
        assert m_f.read().steps == 0 and m_f.read().loss_sum == 0.0 and not bool(m_f.block.any())
    assert torch.equal(blocks[0], blocks[1])


# ---- step level --------------------------------------------------------------------------------------------------------------------
def _trainer(meters, mode):
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_train import _no_dropout, build
    torch.manual_seed(11)
    m = build("512", proj_gamma=0.1).train()
    _no_dropout(m)
    if mode == "frozen":
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            m.freeze()
    tr = Trainer(m, lr=1e-3, meters=meters)
    if mode == "module":
        tr.native_step = False
    return m, tr


@pytest.mark.parametrize("mode", ["native", "module", "frozen"])
def test_trainer_with_meters_equals_twin_without(mode):
    """4 steps, same seed: parameters, losses and last_logits bitwise equal with and without meters; the meters equal the restatement
    applied to each step's logits and loss.  Native step, module path (native_step = False) and frozen features.  The native step
    with meters makes exactly the library calls of the step without, the fused loss entry in place of the plain one (each is two
    launches: include/mnas.h; kernel counts from a rocprofv3 trace of both: profiles/meters_launches.txt)."""
    xs = [C.det_input((8, 3, 64, 64), seed=C.INPUT_SEED + i).cuda() for i in range(4)]
    ts = [((torch.arange(8) * 3 + i) % 10).cuda() for i in range(4)]
    out = {}
    for with_meters in (True, False):
        meters = DeviceMeters((1, 5)) if with_meters else None
        m, tr = _trainer(meters, mode)
        assert (tr._native_head() is not None) == (mode == "native")
        logits = []
        hook = m.register_forward_hook(lambda mod, inp, o: logits.append(o.detach().clone()))
        calls = []
        lib = tr._native_head().lib if mode == "native" else None
        names = ("mnas_head_cross_entropy", "mnas_head_cross_entropy_metrics", "mnas_head_metrics")
        typed = {name: getattr(lib, name) for name in names} if lib is not None else {}
        for name, fn in typed.items():                         # count the calls of the head's loss entry points
            setattr(lib, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(fn, name))
        try:
            losses = []
            for x, t in zip(xs, ts):
                losses.append(tr.step(x, t).clone())
                if mode == "native":
                    logits.append(tr.last_logits.clone())
        finally:
            hook.remove()
            for name, fn in typed.items():
                setattr(lib, name, fn)                         # the typed function objects back in place
        torch.cuda.synchronize()
        out[with_meters] = (tr.flat_p.clone(), losses, logits, meters, calls)
    (p1, l1, z1, meters, c1), (p0, l0, z0, _, c0) = out[True], out[False]
    assert torch.equal(_bits(p1), _bits(p0))
    assert len(z1) == len(z0) == 4
    for a, b in zip(l1 + z1, l0 + z0):
        assert torch.equal(_bits(a), _bits(b))
    if mode == "native":
        assert c0 == ["mnas_head_cross_entropy"] * 4 and c1 == ["mnas_head_cross_entropy_metrics"] * 4
    log = R.StepLog((1, 5))
    for z, t, l in zip(z1, ts, l1):
        log.update(z.cpu().numpy(), t.cpu().numpy(), l.item())
    rec = meters.read()
    print(mode, rec)
    log.check(rec)
    assert rec.steps == 4 and rec.samples == 32 and rec.nonfinite_steps == 0


# ---- validate ----------------------------------------------------------------------------------------------------------------------
def _val_batches(n=3, N=8, classes=10, seed0=40):
    shapes = [(96, 128), (128, 96), (96, 128)]
    out = []
    for i in range(n):
        H, W = shapes[i % len(shapes)]
        out.append((C.det_input((N, 3, H, W), seed=C.INPUT_SEED + seed0 + i).cuda(), ((torch.arange(N) * 7 + i) % classes).cuda()))
    return out


def _hand_loop(m, batches):
    """train.py:556-592 by hand: model.eval(), no_grad, model(x), F.cross_entropy, the restatement"""
    log = R.StepLog((1, 5))
    was = m.training
    m.eval()
    with torch.no_grad():
        for x, t in batches:
            out = m(x)
            log.update(out.cpu().numpy(), t.cpu().numpy(), F.cross_entropy(out, t).item())
    m.train(was)
    return log


def _sync_debug_honoured():
    """does this torch build raise on a synchronising call under set_sync_debug_mode("error")?"""
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_validate_equals_hand_loop_with_one_sync(monkeypatch):
    """3 batches of two rectangular shapes: counts exactly those of the hand-written loop, loss average within the bound
    test_gpu_head.py::test_cross_entropy holds the native loss to against ATen (2e-5 * max(1, |ref|): same logits, only the loss kernel
    differs); train mode restored; BatchNorm running statistics and num_batches_tracked untouched; exactly one host sync -- asserted
    with torch.cuda.set_sync_debug_mode("error") around everything but the final read() where this torch build honours it, and in any
    case by counting Tensor.item / .cpu / .tolist / .numpy calls and torch.cuda.synchronize (all zero before read())."""
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_train import build
    torch.manual_seed(3)
    m = build("512", proj_gamma=0.1).train()               # dropout stays at 0.5: eval mode must switch it off
    tr = Trainer(m, lr=1e-3)
    tr.step(C.det_input((8, 3, 96, 128)).cuda(), (torch.arange(8) % 10).cuda())     # running statistics away from their init
    batches = _val_batches()
    ref = _hand_loop(m, batches)
    assert m.training and m.features.training
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    tr.validate(batches)                                    # programs of both shapes exist from here on
    honoured = _sync_debug_honoured()
    print("torch.cuda.set_sync_debug_mode('error') raises on a synchronising call in this build: %s" % honoured)
    count = {"n": 0, "in_read": False}
    real_read = DeviceMeters.read

    def read(self):
        torch.cuda.set_sync_debug_mode("default")
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

    monkeypatch.setattr(DeviceMeters, "read", read)
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counting(getattr(torch.Tensor, name)))
    monkeypatch.setattr(torch.cuda, "synchronize", counting(torch.cuda.synchronize))
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        rec = tr.validate(batches)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        monkeypatch.undo()
    assert count["n"] == 0, "validate() took %d synchronising calls before read()" % count["n"]
    print("validate:", rec, "| hand loop loss avg %.9g" % ref.loss.avg)
    assert rec.correct == ref.correct and rec.last_correct == ref.last_correct
    assert (rec.samples, rec.steps, rec.last_n, rec.nonfinite_steps) == (24, 3, 8, 0)
    assert abs(rec.loss.avg - ref.loss.avg) <= 2e-5 * max(1.0, abs(ref.loss.avg))
    assert abs(rec.loss.val - ref.loss.val) <= 2e-5 * max(1.0, abs(ref.loss.val))
    assert m.training and all(mod.training for mod in m.modules())
    for k, v in m.named_buffers():
        assert torch.equal(v, bufs[k]), k
    # a caller's meters accumulate across calls; max_batches
    mine = DeviceMeters((1, 3))
    tr.validate(batches, meters=mine, max_batches=2)
    r2 = tr.validate(batches, meters=mine)
    assert r2.steps == 5 and r2.samples == 40 and set(r2.acc) == {1, 3}
    # an exception inside a batch: the modes come back
    def broken():
        yield batches[0]
        raise KeyError("loader died")
    with pytest.raises(KeyError):
        tr.validate(broken())
    assert m.training and all(mod.training for mod in m.modules())
    m.eval()
    tr.validate(batches[:1])
    assert not m.training and not any(mod.training for mod in m.modules())    # an eval-mode model stays in eval mode


def test_validate_module_path_and_transform():
    """a criterion the native loss does not cover (label smoothing) runs as model(x) / criterion / meters.update: same counts, the
    criterion's own loss; `transform` is applied to every input first"""
    from mnasnet_pytorch_amd.train_step import Trainer
    from test_gpu_train import build
    torch.manual_seed(3)
    m = build("512", proj_gamma=0.1).train()
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    tr = Trainer(m, lr=1e-3, criterion=crit)
    assert tr._native_eval_head() is None
    batches = _val_batches()
    ref = _hand_loop(m, batches)
    rec = tr.validate([(x * 2, t) for x, t in batches], transform=lambda x: x * 0.5)
    assert rec.correct == ref.correct and rec.samples == 24
    m.eval()
    with torch.no_grad():
        want = R.Meter()
        for x, t in batches:
            want.update(crit(m(x), t).item(), 8)
    m.train()
    assert rec.loss.avg == want.avg and rec.loss_sum == want.sum


def test_update_is_capturable_in_a_graph():
    """both entry points inside a captured graph (no allocation, no host read of device memory): three replays = three updates"""
    z, t = R.grid_batch(1000, 1.0, 0)
    zc, tc = z.cuda(), t.cuda()
    m = DeviceMeters((1, 5))
    ce = _Loss(R.GRID_N, 1000)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.update(zc, tc)
        ce.fused(zc, tc, m)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        m.update(zc, tc)
        ce.fused(zc, tc, m)
    for _ in range(3):
        graph.replay()
    rec = m.read()
    ref = GOLD["batches"][R.grid_key(1000, 1.0, 0)]
    assert rec.steps == 6 and rec.samples == 6 * R.GRID_N and rec.loss_samples == 3 * R.GRID_N
    assert rec.acc[1].avg == ref["prec1"] and rec.acc[5].avg == ref["prec5"]
