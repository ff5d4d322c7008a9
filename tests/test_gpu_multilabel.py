"""-m gpu: the multi-label branch on the device (csrc/mnas_mlabel.hip, losses.py, metrics.MultiLabelMeters, Trainer.step / validate
with a MultiClassBCELoss) against tests/golden/multilabel.json (what the reference gave) and tests/multilabel_ref.py (the rule).

Bounds.  F1 and the integer counts: exact.  Dice: 4 * 2^-24 -- three fp32 roundings of magnitude <= 1 in 1 + log(2I/U) plus one for a
differing logf.  Loss and gradient: the bounds tests/test_gpu_head.py::test_cross_entropy holds the cross-entropy kernels to, against
an fp64 evaluation of the rule on the same inputs: |loss - ref| <= 2e-5 |ref| and max |dl - ref| < 1e-5 max |ref|.

Per-element bounds (test_bounds*, test_dice_bounds*): every element of dlogits, every row sum, the loss and the focal factor s
inside the brackets of bounds_mlabel.mlabel_intervals (interval propagation through ml_elem as written, expf / log1pf / division at one
ulp; the loss and s from the row sums the device left in the scratch), HardDice inside bounds_mlabel.dice_interval; no element is
excluded.  tests/test_bounds_cpu.py proves on the same inputs that these brackets admit the kernel's arithmetic in every variant
and reject a dropped tail element, a wrong weight, a wrong 1/(N*C), log(1 + ea) for log1pf and the other faults listed there.
MEASURED on an MI355X, worst error / bound: dlogits 0.79, row sums 0.13 (the sparse probes 0.07), loss 0.33, s 0.33, HardDice 0.20."""
import json
import os

import numpy as np
import pytest
import torch

import bounds_mlabel as BM
import cases as C
import intervals as IV
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
    `ok()` checks that they are untouched.  misalign: the weights start 4 bytes past a 16-byte boundary; mis = "z" / "t" / "w" /
    "dl": that pointer alone does (any one of them sends a vector-eligible shape down the scalar path).  rows, s: the row sums
    and the focal factor the device left in the scratch (include/mnas.h: float[N] at byte 8 N, one float at byte 24 N).
    expect: the return code the call must give (then nothing may be written: `untouched()`)."""

    def __init__(self, z, t, w=None, focal=False, gamma=R.FOCUS, balance=R.BALANCE, meters=None, nw=(0, 0, 0), grad=True, misalign=False,
                 mis=None, expect=0, shape=None, null=(), scratch_shift=0):
        lib = L.load()
        N, Cn = z.shape
        self.N, self.Cn = N, Cn
        mis = "w" if misalign else mis
        self.dlo = 1 if mis == "dl" else 0
        self.dl_buf = torch.full((N * Cn + 2 * G + 4,), NAN, device="cuda")
        self.loss_buf = torch.full((2 * G + 1,), NAN, device="cuda")
        self.nb = int(lib.mnas_mlabel_scratch_bytes(N))
        self.scratch = torch.full((self.nb + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        self.keep = []

        def place(x, off):
            buf = torch.zeros(N * Cn + 8, device="cuda")
            buf[off:off + N * Cn] = x.reshape(-1)
            self.keep.append(buf)
            assert (buf.data_ptr() + 4 * off) % 16 == 4 * off
            return buf.data_ptr() + 4 * off
        zptr = place(z, 1) if mis == "z" else z.data_ptr()
        tptr = place(t, 1) if mis == "t" else t.data_ptr()
        wptr = 0 if w is None else place(w, 1 if mis == "w" else 0)
        self.grad = grad
        ptrs = {"logits": zptr, "target": tptr, "scratch": self.scratch.data_ptr() + G + scratch_shift, "loss": self.loss_buf.data_ptr() + 4 * G}
        for k in null:
            ptrs[k] = 0
        assert (self.dl_buf.data_ptr() + 4 * (G + self.dlo)) % 16 == 4 * self.dlo
        cN, cC = (N, Cn) if shape is None else shape
        rc = lib.mnas_mlabel_bce(ptrs["logits"], ptrs["target"], wptr, cN, cC, 1 if focal else 0, float(gamma), float(balance),
                                 ptrs["scratch"], ptrs["loss"], self.dl_buf.data_ptr() + 4 * (G + self.dlo) if grad else 0,
                                 meters.kernel_args(z.device) if meters else 0, nw[0], nw[1], nw[2], L.cur_stream())
        if expect:
            assert rc == expect, rc
        else:
            L.check(rc, "mlabel_bce")
        self.loss = self.loss_buf[G]
        self.dl = self.dl_buf[G + self.dlo:G + self.dlo + N * Cn].view(N, Cn)

    @property
    def rows(self):
        return self.scratch[G + 8 * self.N:G + 12 * self.N].view(torch.float32)

    @property
    def s(self):
        return self.scratch[G + 24 * self.N:G + 24 * self.N + 4].view(torch.float32)[0]

    def untouched(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.dl_buf).all()) and bool(torch.isnan(self.loss_buf).all()) and bool((self.scratch == 0xA5).all())

    def ok(self):
        n = self.N * self.Cn
        assert bool(torch.isnan(self.dl_buf[:G + self.dlo]).all()) and bool(torch.isnan(self.dl_buf[G + self.dlo + n:]).all())
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


# ---- per-element bounds (bounds_mlabel.mlabel_intervals / dice_interval; tests/test_bounds_cpu.py proves that they bite) ------------------------
def _check_bounds(call, z, t, w, focal, gamma, balance, vec, what):
    """every output of one mnas_mlabel_bce call inside its bracket: dlogits and the row sums element by element, the loss and
    (focal) s from the rows the device stored.  z, t, w where the fp64 work shall run (host, or the device for the large case)."""
    N, Cn = z.shape
    dev = z.device
    iv = BM.mlabel_intervals(z, t, w, N, Cn, focal, gamma, balance, vec, rows_dev=call.rows)
    r = {"dlogits": IV.check_interval(call.dl.to(dev), iv["dl"], what + " dlogits", "multi-label dlogits"),
         "rows": IV.check_interval(call.rows.to(dev), iv["rows"], what + " row sums", "multi-label row sums"),
         "loss": IV.check_interval(call.loss.cpu(), iv["loss"], what + " loss", "multi-label loss")}
    if focal:
        r["s"] = IV.check_interval(call.s.cpu(), iv["s"], what + " s", "multi-label focal s")
    return r, iv


def _vec(Cn, mis=None):
    return Cn % 4 == 0 and mis is None


@pytest.mark.parametrize("N,Cn", BM.ML_SHAPES)
def test_bounds(N, Cn):
    """one class; partial waves; the workgroup's second trip on the scalar path (257, 1000 misaligned, 1027: its fifth) and on the
    vector path (1028: second, 2052: third); the batch stage's second and third trip (257, 513 rows).  Every input family of
    bounds_mlabel.mlabel_inputs, all four variants (the confident batch under every focal setting), weights aligned (the vector path
    where C % 4 == 0) and 4 bytes off (the scalar path); guarded buffers.  The fused entry gives the plain one's bits and exact
    meters, as on the older shapes."""
    worst, small = {}, (1.0, 0.0)
    for ki, kind in enumerate(BM.ML_KINDS):
        z, t, w = BM.mlabel_inputs(kind, N, Cn)
        zc, tc, wc = z.cuda(), t.cuda(), w.cuda()
        f1, counts, dice = R.f1_batch(z.numpy(), t.numpy()), R.dice_counts(z.numpy(), t.numpy()), R.hard_dice(z.numpy(), t.numpy())
        for name, weighted, focal in R.LOSS_VARIANTS:
            for gamma, balance in (BM.ML_FOCAL if (focal and kind == "confident") else (BM.ML_FOCAL[ki % 3],)):
                for mis in ((None, "w") if weighted else (None,)):
                    what = "%s %s (%d, %d) gamma %g mis %s" % (kind, name, N, Cn, gamma, mis)
                    m = MultiLabelMeters()
                    a = _Bce(zc, tc, wc if weighted else None, focal, gamma, balance, mis=mis)
                    b = _Bce(zc, tc, wc if weighted else None, focal, gamma, balance, meters=m, nw=(N, N, 3), mis=mis)
                    torch.cuda.synchronize()
                    a.ok(), b.ok()
                    assert torch.equal(_bits(a.loss), _bits(b.loss)) and torch.equal(_bits(a.dl), _bits(b.dl)), what
                    rec = m.read()
                    assert rec.f1.val == f1 and (rec.last_tp, rec.last_fp, rec.last_fn) == counts and rec.loss.val == float(a.loss), what
                    assert abs(rec.hdice.val - dice) <= DICE_TOL and (rec.steps, rec.samples, rec.f1_n) == (1, N, 3), what
                    r, iv = _check_bounds(a, z, t, w if weighted else None, focal, gamma, balance, _vec(Cn, mis), what)
                    for k, v in r.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                    if focal and kind == "confident":
                        small = min(small, (float(iv["b"].mid), float(iv["s"].half / iv["s"].mid.abs())))
                    if kind == "sparse" and weighted and not focal:
                        BM.mlabel_probe_visible(iv, BM.mlabel_live(N, Cn), what)
                        rr = float(((a.rows.cpu().double() - iv["rows"].mid).abs() / iv["row_half"]).max())
                        worst["sparse rows"] = max(worst.get("sparse rows", 0.0), rr)
    print("(%d, %d): worst error / bound %s; smallest confident b %.3g, relative half width of s there %.3g"
          % (N, Cn, ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), small[0], small[1]))


@pytest.mark.parametrize("N,Cn", [(3, 1024), (2, 2052)])
def test_bounds_alignment(N, Cn):
    """a vector-eligible shape: all aligned takes k_mlabel_row<true>; each of z, t, w, dlogits ALONE at element offset 1 takes
    k_mlabel_row<false>.  Each run inside its own path's bracket; dlogits (every element computed alone) bit-equal between the
    paths; the row sums' order differs between the paths, so they are held to their own path's bracket, not to each other.  On
    (3, 1024) the two orders give different bits in every row (tests/test_bounds_cpu.py's emulation, fused and unfused), so a
    misaligned run whose row sums equal the aligned run's did not change path; on (2, 2052) they happen to agree and nothing
    is asserted."""
    z, t, w = BM.mlabel_inputs("scale8", N, Cn)
    zc, tc, wc = z.cuda(), t.cuda(), w.cuda()
    for focal in (False, True):
        base = _Bce(zc, tc, wc, focal).ok()
        _check_bounds(base, z, t, w, focal, R.FOCUS, R.BALANCE, True, "aligned (%d, %d)" % (N, Cn))
        plain = _Bce(zc, tc, wc, False).ok()
        for mis in ("z", "t", "w", "dl"):
            c = _Bce(zc, tc, wc, focal, mis=mis).ok()
            r, iv = _check_bounds(c, z, t, w, focal, R.FOCUS, R.BALANCE, False, "%s off by one element (%d, %d)" % (mis, N, Cn))
            ref = base.dl if not focal else (plain.dl * c.s)           # (focal: s comes from the path's own row sums)
            assert torch.equal(_bits(c.dl), _bits(ref)), (mis, focal)
            if Cn == 1024:      # the dispatch did move: the two lane orders round these rows apart (all three, in the CPU emulation)
                assert not torch.equal(_bits(c.rows), _bits(base.rows)), "%s off by one element: the vector path's row sums" % mis


def test_bounds_scale_second_trip():
    """(1100, 1000) focal, weighted: N*C = 1.1 M > 4096*256, so every lane of k_mlabel_scale's capped grid takes a second trip for
    the elements from 1 048 576 on.  Brackets in fp64 on the device; and separately: every element -- those at and beyond the cap
    among them -- is the unscaled gradient times the device's s, rounded once, to the bit (scaled exactly once)."""
    N, Cn = BM.ML_BIG
    cap = 4096 * 256
    z, t, w = BM.mlabel_inputs("scale8", N, Cn)
    zc, tc, wc = z.cuda(), t.cuda(), w.cuda()
    gamma, balance = BM.ML_FOCAL[1]
    a = _Bce(zc, tc, wc, True, gamma, balance).ok()
    plain = _Bce(zc, tc, wc, False).ok()
    r, _ = _check_bounds(a, zc, tc, wc, True, gamma, balance, True, "(1100, 1000) focal")
    once = (plain.dl * a.s).reshape(-1)
    got = a.dl.reshape(-1)
    assert float(a.s) != 1.0 and N * Cn > cap
    assert torch.equal(_bits(got[cap:]), _bits(once[cap:])), "elements from 4096*256 on are not scaled exactly once"
    assert torch.equal(_bits(got[:cap]), _bits(once[:cap]))
    assert (gamma, balance) == (R.FOCUS, R.BALANCE)
    _check_loss(a, z, t, w, True, "(1100, 1000) focal")                 # (the older tolerances, beside the brackets)
    print("(1100, 1000) focal: worst error / bound %s" % ", ".join("%s %.3f" % kv for kv in sorted(r.items())))


def _dice_batch(N, Cn, I, fp, fn, weak=0):
    """logits / targets on the device with I predicted-and-true, fp predicted-only and fn true-only elements; `weak` of the I
    sit at z = 0.5: predicted under threshold 0.5, not under 0.7"""
    z = torch.full((N * Cn,), -3.0, device="cuda")
    t = torch.zeros(N * Cn, device="cuda")
    z[:I + fp] = 3.0
    z[:weak] = 0.5
    t[:I] = 1.0
    t[I + fp:I + fp + fn] = 1.0
    return z.view(N, Cn), t.view(N, Cn)


def _hard_dice(z, t, thr_logit, deduct, expect=0, null=()):
    lib = L.load()
    N, Cn = z.shape
    out = torch.full((2 * G + 1,), NAN, device="cuda")
    nb = int(lib.mnas_mlabel_scratch_bytes(N))
    scratch = torch.full((nb + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    p = {"z": z.data_ptr(), "t": t.data_ptr(), "scratch": scratch.data_ptr() + G, "out": out.data_ptr() + 4 * G}
    for k in null:
        p[k] = 0
    rc = lib.mnas_mlabel_hard_dice(p["z"], p["t"], N, Cn, float(thr_logit), deduct, p["scratch"], p["out"], L.cur_stream())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect and bool(torch.isnan(out).all()) and bool((scratch == 0xA5).all())
        return None
    L.check(rc, "hard_dice")
    assert bool(torch.isnan(out[:G]).all()) and bool(torch.isnan(out[G + 1:]).all())
    assert bool((scratch[:G] == 0xA5).all()) and bool((scratch[G + nb:] == 0xA5).all())
    return out[G].cpu()


@pytest.mark.parametrize("N,Cn,I,fp,fn,weak", [(1, 7, 7, 0, 0, 0), (100, 1000, 18394, 31606, 31606, 0), (100, 1001, 18394, 31606, 31607, 0),
                                               (7, 33, 40, 50, 90, 11), (3, 5, 0, 5, 9, 0), (1, 1, 1, 0, 0, 0)])
def test_dice_bounds(N, Cn, I, fp, fn, weak):
    """2I == U: exactly 1.0; 2I/U = 0.36788 and 0.3678763, either side of 1/e (the clamp at 0); deduct pushing the value above 1
    (clamped); thresholds 0.5 and 0.7 (the `weak` hits drop out under 0.7); nothing hit: 0.  Counts from numpy (dice_counts);
    the old DICE_TOL assertion beside the bracket."""
    z, t = _dice_batch(N, Cn, I, fp, fn, weak)
    zn, tn = z.cpu().numpy(), t.cpu().numpy()
    for th in (0.5, 0.7):
        thr = float(np.log(th / (1 - th)))
        tp, fp_, fn_ = R.dice_counts(zn, tn, thr)
        assert (tp, fp_, fn_) == ((I, fp, fn) if th == 0.5 else (I - weak, fp, fn + weak))
        for deduct in (0, 1):
            got = _hard_dice(z, t, thr, deduct)
            iv = BM.dice_interval(tp, tp + fp_, tp + fn_, deduct)
            r = IV.check_interval(got, iv, "HardDice %r threshold %g deduct %d" % ((N, Cn, I, fp, fn), th, deduct), "HardDice")
            assert abs(float(got) - R.hard_dice(zn, tn, thr, bool(deduct))) <= DICE_TOL
            if tp > 0 and fp_ == 0 and fn_ == 0:
                assert float(got) == 1.0                                  # 2I == U: 1 + logf(1); with deduct 1 + log 2, clamped
            if tp == 0:
                assert float(got) == 0.0
    if (I, fp, fn) == (18394, 31606, 31606):
        assert 0.0 < float(_hard_dice(z, t, 0.0, 0)) < 1e-5
    if (I, fp, fn) == (18394, 31606, 31607):
        assert float(_hard_dice(z, t, 0.0, 0)) == 0.0


def test_dice_bounds_rounded_conversion():
    """4100 x 4100 (16.8 M elements built on the device: under 0.1 s, so the size is not reduced), all predicted and true but 3 + 2: 2I = 33 619 990 > 2^25 and U = 33 619 995 are no
    fp32 numbers, so (float)(2I) and (float)U round.  The mnas_mlabel_hard_dice entry only; the counts are known by construction."""
    N = Cn = 4100
    I, fp, fn = N * Cn - 5, 2, 3
    z, t = _dice_batch(N, Cn, I, fp, fn)
    assert float(torch.tensor(float(2 * I)).float()) != 2 * I and 2 * I > 2 ** 25
    for deduct in (0, 1):
        got = _hard_dice(z, t, 0.0, deduct)
        r = IV.check_interval(got, BM.dice_interval(I, I + fp, I + fn, deduct), "HardDice 4100 x 4100 deduct %d" % deduct, "HardDice")
        print("HardDice 4100 x 4100 deduct %d: %r, error / bound %.3f" % (deduct, float(got), r))


def test_rejects_write_nothing():
    """every refused call returns MNAS_EINVAL and leaves the NaN / 0xA5 guards and the meter block as they were"""
    z, t, w = BM.mlabel_inputs("scale8", 3, 8)
    zc, tc, wc = z.cuda(), t.cuda(), w.cuda()
    m = MultiLabelMeters()
    m.update(zc, tc)
    torch.cuda.synchronize()
    block = m.block.clone()
    E = L.EINVAL
    kw = dict(meters=m, nw=(3, 3, 3), expect=E)
    cases = [dict(shape=(0, 8)), dict(shape=(-1, 8)), dict(shape=(3, 0)), dict(shape=(3, -2)), dict(null=("logits",)), dict(null=("target",)),
             dict(null=("scratch",)), dict(null=("loss",)), dict(scratch_shift=8), dict(focal=True, gamma=0.5), dict(focal=True, gamma=NAN),
             dict(nw=(-1, 3, 3)), dict(nw=(3, -1, 3)), dict(nw=(3, 3, -1))]
    for c in cases:
        _Bce(zc, tc, wc, **{**kw, **c}).untouched()
        assert torch.equal(m.block, block), c
    for c in (dict(null=("z",)), dict(null=("t",)), dict(null=("scratch",)), dict(null=("out",))):
        _hard_dice(zc, tc, 0.0, 0, expect=E, **c)
    _hard_dice(zc, tc, NAN, 0, expect=E)
    _hard_dice(zc[:0], tc[:0], 0.0, 0, expect=E)
    assert torch.equal(m.block, block)
    _Bce(zc, tc, wc, meters=m, nw=(3, 3, 3)).ok()                       # ... and the same arguments, valid, do run
    assert not torch.equal(m.block, block)


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
