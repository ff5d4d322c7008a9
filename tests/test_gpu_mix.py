"""-m gpu: label smoothing and batch mixing on the MI355X.  The soft-target cross-entropy kernels (csrc/mnas_head.hip) through the
C ABI against torch fp64 on the CPU (tests/mix_ref.py), with the bounds tests/test_gpu_head.py::test_cross_entropy holds the plain
loss to; the mix kernel (csrc/mnas_imgm.hip) byte for byte against the numpy restatement, inside canary bytes; Trainer steps on
mixed batches against the module path, against nn.CrossEntropyLoss (bit-equal without smoothing) and against a batch mixed on the
host (bit-equal)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bounds_tail as BT
import cases as C
import gpu_util as G
import intervals as IV
import metrics_ref as MR
import mix_ref as R
from cases import O
from gpu_util import relerr
from mnasnet_pytorch_amd import _lib as L

pytestmark = pytest.mark.gpu
PAD = 4096                                     # canary bytes on each side of an output
GUARD = 1024                                   # NaN floats on each side of dlogits


# ---- the loss kernels --------------------------------------------------------------------------------------------------------------
class _Soft:
    """the raw mnas_head_cross_entropy_soft call with its own scratch; dlogits inside a NaN-filled, guarded buffer"""

    def __init__(self, N, Cn):
        self.N, self.Cn = N, Cn
        self.rows = torch.empty(N, device="cuda")
        self.loss = torch.full((), 12345.0, device="cuda")
        self.buf = torch.full((N * Cn + 2 * GUARD,), float("nan"), device="cuda")
        self.bad = torch.zeros(1, dtype=torch.int32, device="cuda")

    @property
    def dl(self):
        return self.buf[GUARD:GUARD + self.N * self.Cn].view(self.N, self.Cn)

    def run(self, z, a, b, lam, eps, meters=None, grad=True, ignore=-100):
        self.buf.fill_(float("nan"))
        self.bad.zero_()
        ks, nk, ranks, blk = (None, 0, 0, 0) if meters is None else meters.kernel_args(self.N, z.device)
        L.check(L.load().mnas_head_cross_entropy_soft(z.data_ptr(), a.data_ptr(), L.ptr(b), L.ptr(lam), eps, self.N, self.Cn, ignore,
                                                      self.rows.data_ptr(), self.loss.data_ptr(), self.dl.data_ptr() if grad else 0,
                                                      self.bad.data_ptr(), ks, nk, ranks, blk, L.cur_stream()))
        host = self.buf.cpu()
        assert bool(torch.isnan(host[:GUARD]).all()) and bool(torch.isnan(host[GUARD + self.N * self.Cn:]).all()), "write outside dlogits"
        return float(self.loss), host[GUARD:GUARD + self.N * self.Cn].view(self.N, self.Cn), int(self.bad)


def _targets(N, Cn):
    """{variant: (a, b or None, lam or None)} on the CPU"""
    i = torch.arange(N)
    a = (i * 7 + 3) % Cn
    b = (i * 5 + 1) % Cn
    hard = torch.tensor([0.0, 0.5, 1.0, 0.3, 0.8125, 0.49999997])[i % 6]          # exactly 0, 0.5 and 1 among them
    a_ign, b_ign = a.clone(), b.clone()
    a_ign[::3] = -100
    b_ign[1::3] = -100
    none = torch.full((N,), -100)
    return {
        "no mixing": (a, None, None),
        "no mixing, rows ignored": (a_ign, None, None),
        "one lam per batch": (a, b, torch.full((N,), 0.3)),
        "lam per row": (a, b, hard),
        "a == b": (a, a.clone(), hard.flip(0).contiguous()),
        "a ignored": (a_ign, b, hard),
        "b ignored": (a, b_ign, hard),
        "a or b ignored": (a_ign, b_ign, hard),
        "b given, lam null": (a, b, None),
        "all ignored": (none, None, None),
        "all ignored, mixing": (a, none, hard),
    }


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N,Cn", [(1, 1), (7, 10), (33, 257), (256, 1000)])
def test_soft_cross_entropy_against_fp64(N, Cn, eps):
    z = O.det_uniform((N, Cn), 11) * 4
    zc = z.cuda()
    ce = _Soft(N, Cn)
    for name, (a, b, lam) in _targets(N, Cn).items():
        ref, gref = R.soft_ce(z, a, b, lam if b is not None else None, eps)
        dev = [None if t is None else t.cuda() for t in (a, b, lam)]
        loss, dl, bad = ce.run(zc, *dev, eps)
        msg = (name, N, Cn, eps, loss, float(ref))
        assert bad == 0, msg
        assert not bool(torch.isnan(dl).any()), msg                       # every element written
        if torch.isnan(ref):                                              # no row counted: 0 / 0
            assert loss != loss and bool((dl == 0).all()), msg
            continue
        print("%-24s N %3d C %4d eps %.1f  loss %.8f ref %.8f  |d| %.2e  relerr(dlogits) %.2e"
              % (name, N, Cn, eps, loss, float(ref), abs(loss - float(ref)), relerr(dl, gref)))
        assert abs(loss - float(ref)) < 2e-5 * max(1.0, abs(float(ref))), msg
        assert relerr(dl, gref) < 1e-5, msg
        # forward only: the same loss, nothing written
        loss2, dl2, _ = ce.run(zc, *dev, eps, grad=False)
        assert loss2 == loss and bool(torch.isnan(dl2).all()), msg


@pytest.mark.parametrize("N,Cn", [(7, 10), (33, 257)])
def test_soft_cross_entropy_refuses_bad_labels_and_weights(N, Cn):
    zc = (O.det_uniform((N, Cn), 12) * 4).cuda()
    ce = _Soft(N, Cn)
    a, b, lam = _targets(N, Cn)["one lam per batch"]

    def run(a_, b_, lam_):
        return ce.run(zc, a_.cuda(), None if b_ is None else b_.cuda(), None if lam_ is None else lam_.cuda(), 0.1)

    loss, _, bad = run(a, b, lam)
    assert bad == 0 and loss == loss
    for what, val in (("a", Cn), ("a", -1), ("b", Cn), ("b", -7), ("lam", 1.5), ("lam", float("nan")), ("lam", -0.25),
                      ("lam", float("inf"))):
        aa, bb, ll = a.clone(), b.clone(), lam.clone()
        {"a": aa, "b": bb, "lam": ll}[what][2] = val
        loss, dl, bad = run(aa, bb, ll)
        assert bad == 1 and loss != loss, (what, val, loss, bad)
        assert bool((dl[2] == 0).all()) and not bool(torch.isnan(dl).any())       # the refused row has no gradient
    aa = a.clone()
    aa[0] = Cn + 5
    loss, _, bad = run(aa, None, None)                                            # without mixing as well
    assert bad == 1 and loss != loss
    # an ignored row hides a refused partner label: it is not looked at
    aa, bb = a.clone(), b.clone()
    aa[3], bb[3] = -100, Cn
    loss, _, bad = run(aa, bb, lam)
    assert bad == 0 and loss == loss
    # arguments refused before any launch
    lib = L.load()
    args = (ce.rows.data_ptr(), ce.loss.data_ptr(), 0, ce.bad.data_ptr(), None, 0, 0, 0, L.cur_stream())
    for eps in (-0.1, 1.5, float("nan")):
        assert lib.mnas_head_cross_entropy_soft(zc.data_ptr(), a.cuda().data_ptr(), 0, 0, eps, N, Cn, -100, *args) == L.EINVAL
    assert lib.mnas_head_cross_entropy_soft(zc.data_ptr(), 0, 0, 0, 0.1, N, Cn, -100, *args) == L.EINVAL


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_soft_cross_entropy_meters_rank_the_dominant_label(eps):
    """with meters: loss, dlogits and flag bit-equal to the call without; counts and loss sums exactly the restatement's meter fed
    the label with the larger weight (a when lam >= 0.5), ignored rows wrong"""
    from mnasnet_pytorch_amd.metrics import DeviceMeters
    log = MR.StepLog((1, 5))
    meters = DeviceMeters((1, 5))
    for N, Cn in [(7, 10), (33, 257), (256, 1000)]:
        z, t = MR.grid_batch(Cn, 1.0, 3, N)
        ce = _Soft(N, Cn)
        for name, (a, b, lam) in _targets(N, Cn).items():
            if name.startswith("all ignored"):
                continue
            a = torch.where(a >= 0, torch.where(torch.arange(N) % 2 == 0, t, a), a)       # half the rows aim at a boosted logit
            dev = [None if v is None else v.cuda() for v in (a, b, lam)]
            plain = ce.run(z.cuda(), *dev, eps)
            fused = ce.run(z.cuda(), *dev, eps, meters=meters)
            assert fused[0] == plain[0] and torch.equal(fused[1], plain[1]) and fused[2] == plain[2] == 0, name
            bb = a if b is None else b
            ll = torch.ones(N) if (b is None or lam is None) else lam
            dom = torch.where((a == -100) | (bb == -100), torch.full_like(a, -100), R.dominant(a, bb, ll))
            log.update(z.numpy(), dom.numpy(), fused[0], ignore_index=-100)
    rec = meters.read()
    print(rec)
    log.check(rec)
    assert 0 < rec.correct[1] < rec.correct[5] < rec.samples


# ---- per-element brackets (bounds_tail.ce_intervals: interval propagation through k_head_ce_soft's own roundings) ----------------------
def _lam_variants(N):
    i = torch.arange(N)
    per_row = torch.tensor([0.0, 0.5, 1.0, 0.3, 0.8125, 0.49999997])[i % 6]
    out = [("lam %g" % v, True, torch.full((N,), v)) for v in (0.0, 1.0, 0.5, 0.3)]
    return out + [("lam per row", True, per_row), ("tb null", False, None), ("lam null", True, None)]


def _soft_labels(N, Cn, how):
    a, b = BT.ce_targets(N, Cn)
    b = torch.where(torch.arange(N) % 4 == 1, a, b)                  # rows with a == b among the others
    return BT.ce_ignore(a, how), b


def _plain(z, t):
    N, Cn = z.shape
    rows, loss = torch.empty(N, device="cuda"), torch.empty((), device="cuda")
    dl = torch.full((N, Cn), float("nan"), device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(L.load().mnas_head_cross_entropy(z.data_ptr(), t.data_ptr(), N, Cn, -100, rows.data_ptr(), loss.data_ptr(), dl.data_ptr(),
                                             bad.data_ptr(), L.cur_stream()))
    return rows.cpu(), dl.cpu(), loss.cpu()


@pytest.mark.parametrize("N,Cn", BT.CE_SIZES)
def test_soft_cross_entropy_per_element_bracket(N, Cn):
    """EVERY dlogits element, every loss row and the mean of k_head_ce_soft inside bounds_tail.ce_intervals' bracket: eps 0 / 0.1 / 1
    x lam 0 / 1 / 0.5 / 0.3 / per row / tb NULL / lam NULL for every kind of logit row and every way of ignoring rows (at
    N C > 10000 the way rows are ignored cycles over the 21 settings instead), rows with a == b in every batch; the same call
    with meters gives the same bits."""
    from mnasnet_pytorch_amd.metrics import DeviceMeters
    meters = DeviceMeters((1, 5))
    ce = _Soft(N, Cn)
    settings = [(eps, v) for eps in (0.0, 0.1, 1.0) for v in _lam_variants(N)]
    if N * Cn > 10000:
        runs = [(k, BT.CE_IGNORE[(i + j) % 4], s) for i, k in enumerate(BT.CE_ROWS) for j, s in enumerate(settings)]
    else:
        runs = [(k, h, s) for k in BT.CE_ROWS for h in BT.CE_IGNORE for s in settings]
    worst = 0.0
    for kind, how, (eps, (name, mixing, lam)) in runs:
        z = BT.ce_logits(kind, N, Cn)
        a, b = _soft_labels(N, Cn, how)
        b = b if mixing else None
        what = "soft ce %s / %s / eps %g / %s (%d, %d)" % (kind, how, eps, name, N, Cn)
        dev = [None if t is None else t.cuda() for t in (a, b, lam)]
        loss, dl, bad = ce.run(z.cuda(), *dev, eps)
        rows, loss_t = ce.rows.cpu(), ce.loss.cpu()
        iv = BT.ce_intervals(z, a, b, lam, eps)
        assert bad == 0, what
        assert bool((dl[~iv["valid"]] == 0).all()) and bool((rows[~iv["valid"]] == 0).all()), what
        r = [IV.check_interval(dl, iv["dl"], what + " dlogits", "soft cross-entropy"), IV.check_interval(rows, iv["rows"], what + " rows", "soft cross-entropy"),
             BT.check_ce_mean(loss_t, rows, iv["count"], what + " mean", "cross-entropy mean")]
        if iv["count"] == 0:
            assert loss != loss and bool((dl == 0).all()), what
        worst = max(worst, *r)
        loss2, dl2, bad2 = ce.run(z.cuda(), *dev, eps, meters=meters)
        G.bits_equal(dl2, dl, what + " dlogits with meters")
        G.bits_equal(ce.rows.cpu(), rows, what + " rows with meters")
        G.bits_equal(ce.loss.cpu(), loss_t, what + " loss with meters")
    print("soft cross-entropy (%d, %d): %d runs, worst error / bracket %.3f" % (N, Cn, len(runs), worst),
          {k: round(v, 4) for k, v in IV.WORST.items() if "entropy" in k})
    assert worst <= 1.0


@pytest.mark.parametrize("N,Cn", BT.CE_SIZES)
def test_soft_cross_entropy_without_smoothing_is_the_plain_kernel(N, Cn):
    """eps = 0, tb NULL: loss_rows, dlogits and the mean equal k_head_ce's bit for bit -- for finite logits, and for rows with
    -inf at classes that are not labels (a masked class): without smoothing such a row has the plain kernel's finite loss."""
    ce = _Soft(N, Cn)
    for kind in BT.CE_ROWS:
        z = BT.ce_logits(kind, N, Cn).cuda()
        for how in BT.CE_IGNORE:
            t = BT.ce_ignore(BT.ce_targets(N, Cn)[0], how).cuda()
            rows_p, dl_p, loss_p = _plain(z, t)
            loss, dl, bad = ce.run(z, t, None, None, 0.0)
            what = "%s / %s (%d, %d)" % (kind, how, N, Cn)
            assert bad == 0, what
            G.bits_equal(ce.rows.cpu(), rows_p, what + " loss rows")
            G.bits_equal(dl, dl_p, what + " dlogits")
            G.bits_equal(ce.loss.cpu(), loss_p, what + " loss")
            if int((t != -100).sum()) > 0:
                assert bool(torch.isfinite(loss_p)) and bool(torch.isfinite(rows_p).all()), what


# ---- the mix kernel ----------------------------------------------------------------------------------------------------------------
def _items(draws):
    from mnasnet_pytorch_amd.mixing import DeviceMix, MixDraw
    return DeviceMix.items([MixDraw(*d) for d in draws])


def _mix_run(x, draws, in_off=0, out_off=0, arr=None):
    """mnas_img_mix of the host batch x into the middle of a canary buffer, twice over two fill bytes -> output on the host"""
    lib = L.load()
    n, _, h, w = x.shape
    size = x.size
    arr = _items(draws) if arr is None else arr
    items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
    xin = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    xin[in_off:in_off + size].copy_(torch.from_numpy(x.reshape(-1)))
    outs = []
    for fill in (0x5A, 0xA5):
        buf = torch.full((size + 2 * PAD + 64,), fill, dtype=torch.uint8, device="cuda")
        o = PAD + out_off
        L.check(lib.mnas_img_mix(items.data_ptr(), n, h, w, xin.data_ptr() + in_off, buf.data_ptr() + o, L.cur_stream()))
        b = buf.cpu()
        assert bool((b[:o] == fill).all()) and bool((b[o + size:] == fill).all()), "write outside the output"
        outs.append(b[o:o + size].view(n, 3, h, w).numpy().copy())
    assert bool((xin[in_off:in_off + size].cpu() == torch.from_numpy(x.reshape(-1))).all()), "the input was written"
    return outs


def _templates(h, w):
    """(mode, w16, box) a shape's images cycle through: every Mixup weight, every kind of box, the copy"""
    out = [(R.NONE, 65536, (0, 0, 0, 0))]
    out += [(R.MIXUP, w16, (0, 0, 0, 0)) for w16 in (0, 1, 32768, 65535, 65536, 12345)]
    cy, cx = h // 2, w // 2
    boxes = [(0, 0, 0, 0), (cy, cx, cy, cx), (0, 0, h, w), (cy, cx, cy + 1, cx + 1),              # empty, empty inside, full, a pixel
             (0, 0, max(1, h // 3), w), (h - max(1, h // 3), 0, h, w),                            # flush with top, bottom
             (0, 0, h, max(1, w // 3)), (0, w - max(1, w // 3), h, w),                            # flush with left, right
             (min(1, h - 1), min(3, w - 1), h, max(min(3, w - 1), w - 2)),                        # edges off the 16-byte grid
             (h // 4, min(5, w - 1), max(h // 4, h - 1), max(min(5, w - 1), (2 * w) // 3 + 1 if w > 2 else w)),
             (h - 1, w - 1, h, w), (0, 0, 1, 1)]                                                  # the last and the first byte
    out += [(R.CUTMIX, 65536, tuple(int(v) for v in bx)) for bx in boxes]
    return out


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (3, 5, 7), (4, 16, 16), (2, 17, 33), (5, 64, 48), (2, 224, 224)])
def test_mix_kernel_bytes(n, h, w):
    rng = np.random.default_rng(n * 1000 + h)
    x = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    x[0, 0].flat[0], x[-1, -1].flat[-1] = 255, 0
    pool = _templates(h, w)
    for bx in (t[2] for t in pool):
        assert 0 <= bx[0] <= bx[2] <= h and 0 <= bx[1] <= bx[3] <= w, bx
    rounds = -(-len(pool) // n) + 1
    seen = set()
    for r in range(rounds):
        draws = []
        for k in range(n):
            mode, w16, box = pool[(r * n + k) % len(pool)]
            draws.append((mode, (k + 1 + r) % n, w16, box, 1.0))
            seen.add(mode)
        want = R.mix_batch(x, draws)
        for got in _mix_run(x, draws):
            assert np.array_equal(got, want), (n, h, w, r, draws)
    assert seen == {R.NONE, R.MIXUP, R.CUTMIX}
    # partner == self: the image itself, whatever the mode
    draws = [(pool[(3 * k + 1) % len(pool)][0], k) + pool[(3 * k + 1) % len(pool)][1:] + (1.0,) for k in range(n)]
    for got in _mix_run(x, draws):
        assert np.array_equal(got, x)
    # unaligned bases: the same bytes through the byte path
    draws = [(pool[(5 * k + 2) % len(pool)][0], (k + 1) % n) + pool[(5 * k + 2) % len(pool)][1:] + (1.0,) for k in range(n)]
    draws[0] = (R.MIXUP, n - 1, 12345, (0, 0, 0, 0), 1.0)
    want = R.mix_batch(x, draws)
    for in_off, out_off in ((3, 0), (0, 1), (16, 16), (5, 9)):
        for got in _mix_run(x, draws, in_off, out_off):
            assert np.array_equal(got, want), (in_off, out_off)


def test_mix_kernel_permutation_and_modes_in_one_batch():
    """a 3-cycle and a swap: every partner's bytes are the INPUT's (a pass in place would have overwritten them); the three modes side
    by side"""
    rng = np.random.default_rng(77)
    for h, w in [(64, 48), (9, 11)]:
        x = rng.integers(0, 256, (5, 3, h, w), dtype=np.uint8)
        partners = [1, 2, 0, 4, 3]
        kinds = [(R.MIXUP, 20000, (0, 0, 0, 0)), (R.CUTMIX, 65536, (2, 3, h - 1, w - 2)), (R.MIXUP, 40000, (0, 0, 0, 0)),
                 (R.CUTMIX, 65536, (0, 0, h, w)), (R.NONE, 65536, (0, 0, 0, 0))]
        draws = [(m, p, w16, bx, 1.0) for (m, w16, bx), p in zip(kinds, partners)]
        want = R.mix_batch(x, draws)
        assert np.array_equal(want[3], x[4]) and np.array_equal(want[4], x[4])
        for got in _mix_run(x, draws):
            assert np.array_equal(got, want)


def test_mix_kernel_refused_item_writes_nothing_and_overlap_is_einval():
    lib = L.load()
    rng = np.random.default_rng(78)
    n, h, w = 4, 32, 48
    x = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    good = [(R.MIXUP, 1, 30000, (0, 0, 0, 0), 1.0), (R.CUTMIX, 2, 65536, (3, 5, 20, 41), 1.0), (R.NONE, 2, 65536, (0, 0, 0, 0), 1.0),
            (R.CUTMIX, 0, 65536, (0, 0, h, 7), 1.0)]
    want = R.mix_batch(x, good)
    for bad_at, field, val in [(0, "mode", 3), (1, "mode", -1), (0, "partner", n), (3, "partner", -1), (0, "w16", 65537), (2, "w16", -1),
                               (1, "y1", h + 1), (1, "x1", w + 1), (1, "y0", 21), (1, "x0", 42), (3, "y0", -1), (3, "x0", -1),
                               (2, "reserved", 1)]:
        arr = _items(good)
        setattr(arr[bad_at], field, val)
        assert lib.mnas_img_mix_check(arr, n, h, w) == L.EINVAL, (field, val)
        for got, fill in zip(_mix_run(x, None, arr=arr), (0x5A, 0xA5)):
            for k in range(n):
                if k == bad_at:
                    assert bool((got[k] == fill).all()), (field, val, k)
                else:
                    assert np.array_equal(got[k], want[k]), (field, val, k)
    # in == out, and a partial overlap on either side: refused, nothing launched, nothing written
    items = torch.frombuffer(bytearray(_items(good)), dtype=torch.uint8).cuda()
    buf = torch.from_numpy(np.concatenate([x.reshape(-1), x.reshape(-1)])).cuda()
    before = buf.clone()
    for d_in, d_out in ((0, 0), (0, 16), (16, 0), (0, x.size - 1), (x.size - 1, 0)):
        assert lib.mnas_img_mix(items.data_ptr(), n, h, w, buf.data_ptr() + d_in, buf.data_ptr() + d_out, L.cur_stream()) == L.EINVAL
    assert lib.mnas_img_mix(items.data_ptr(), n, h, w, buf.data_ptr(), buf.data_ptr() + x.size, L.cur_stream()) == 0     # adjacent is fine
    torch.cuda.synchronize()
    assert torch.equal(buf[:x.size], before[:x.size]) and np.array_equal(buf[x.size:].cpu().numpy().reshape(x.shape), want)


def test_device_mix_apply_returns_bytes_and_target():
    from mnasnet_pytorch_amd import DeviceMix, MixedTarget
    import random
    rng = np.random.default_rng(79)
    x = rng.integers(0, 256, (6, 3, 40, 56), dtype=np.uint8)
    t = torch.tensor([4, 1, 9, 0, 7, 3])
    for seed, kw in enumerate([dict(mixup_alpha=0.4), dict(cutmix_alpha=1.0), dict(mixup_alpha=0.4, cutmix_alpha=1.0, per_sample=True, prob=0.7)]):
        mix = DeviceMix(**kw)
        random.seed(seed)
        draws = mix.describe(6, 40, 56)
        random.seed(seed)
        xm, mt = mix(torch.from_numpy(x).cuda(), t.cuda())
        assert isinstance(mt, MixedTarget) and xm.dtype == torch.uint8 and xm.shape == (6, 3, 40, 56)
        assert np.array_equal(xm.cpu().numpy(), R.mix_batch(x, [tuple(d) for d in draws]))
        assert torch.equal(mt.a.cpu(), t) and torch.equal(mt.b.cpu(), t[[d.partner for d in draws]])
        assert torch.equal(mt.lam.cpu(), torch.tensor([d.lam for d in draws], dtype=torch.float32))
    with pytest.raises(ValueError):
        DeviceMix.apply(torch.from_numpy(x).cuda(), t.cuda(), [draws[0]._replace(partner=6)] + draws[1:])       # the host check
    with pytest.raises(ValueError):
        DeviceMix.apply(torch.from_numpy(x).cuda().float(), t.cuda(), draws)


# ---- Trainer -----------------------------------------------------------------------------------------------------------------------
def _model(u8=False):
    from test_gpu_train import build, _no_dropout
    m = build("512", proj_gamma=0.1).train()
    _no_dropout(m)
    if u8:
        m.normalize_on_device()
    return m


def _mixed(n=4):
    from mnasnet_pytorch_amd import MixedTarget
    a = torch.tensor([1, 3, 5, 7, 2, 9, 0, 4][:n])
    return MixedTarget(a, a.roll(1), torch.tensor([0.3, 0.5, 1.0, 0.0, 0.75, 0.25, 0.6, 0.45][:n])).to("cuda")


def test_mixed_native_step_matches_module_path():
    """(a) MixCrossEntropyLoss(0.1) on a MixedTarget: the native step against model(x) / criterion / backward, two steps, with the
    bounds of test_gpu_head.py::test_native_step_matches_module_path"""
    from mnasnet_pytorch_amd import MixCrossEntropyLoss
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = _mixed()
    res = []
    for native in (True, False):
        tr = Trainer(_model(), lr=1e-3, criterion=MixCrossEntropyLoss(0.1))
        tr.native_step = native
        losses = [float(tr.step(x, t)) for _ in range(2)]
        res.append((losses, tr.flat_p.clone()))
        assert (tr._native_head() is not None) == native
    print("losses native %r module %r relerr(params) %.3e" % (res[0][0], res[1][0], relerr(res[0][1].cpu(), res[1][1].cpu())))
    assert np.allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-6)
    assert relerr(res[0][1].cpu(), res[1][1].cpu()) < 1e-5
    # a MixedTarget for a criterion that cannot take one: refused before anything is launched
    tr = Trainer(_model(), lr=1e-3)
    before = tr.flat_p.clone()
    with pytest.raises(TypeError):
        tr.step(x, t)
    assert torch.equal(tr.flat_p, before) and tr.step_count == 0


def test_no_smoothing_int_targets_step_bit_equal_to_cross_entropy():
    """(b) MixCrossEntropyLoss() on class indices steps bit for bit as nn.CrossEntropyLoss() does"""
    from mnasnet_pytorch_amd import MixCrossEntropyLoss
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = torch.tensor([1, 3, 5, 7]).cuda()
    res = []
    for crit in (MixCrossEntropyLoss(), torch.nn.CrossEntropyLoss()):
        tr = Trainer(_model(), lr=1e-3, criterion=crit)
        assert tr._native_head() is not None
        losses = [tr.step(x, t).clone() for _ in range(2)]
        res.append((losses, tr.flat_p.clone()))
    assert torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0]))


def test_step_on_device_mixed_batch_bit_equal_to_host_mixed():
    """(c) a uint8 batch mixed by DeviceMix.apply from explicit draws, then stepped, against the same step on the batch the
    restatement mixed on the host: same bytes, bit-equal loss and parameters"""
    from mnasnet_pytorch_amd import DeviceMix, MixCrossEntropyLoss, MixedTarget
    from mnasnet_pytorch_amd.mixing import MixDraw, cutmix_box
    from mnasnet_pytorch_amd.train_step import Trainer
    rng = np.random.default_rng(80)
    x = rng.integers(0, 256, (4, 3, 64, 64), dtype=np.uint8)
    t = torch.tensor([1, 3, 5, 7])
    box, eff = cutmix_box(64, 64, 0.6, 20, 50)
    draws = [MixDraw(R.MIXUP, 2, 12345, (0, 0, 0, 0), 12345 / 65536.0), MixDraw(R.CUTMIX, 3, 65536, box, eff),
             MixDraw(R.NONE, 2, 65536, (0, 0, 0, 0), 1.0), MixDraw(R.MIXUP, 0, 50000, (0, 0, 0, 0), 50000 / 65536.0)]
    res = []
    for route in ("device", "host"):
        if route == "device":
            xm, mt = DeviceMix.apply(torch.from_numpy(x).cuda(), t.cuda(), draws)
        else:
            xm = torch.from_numpy(R.mix_batch(x, [tuple(d) for d in draws])).cuda()
            mt = MixedTarget(t, t[[d.partner for d in draws]], torch.tensor([d.lam for d in draws], dtype=torch.float32)).to("cuda")
        tr = Trainer(_model(u8=True), lr=1e-3, criterion=MixCrossEntropyLoss(0.1))
        assert tr._native_head() is not None
        loss = tr.step(xm, mt)
        torch.cuda.synchronize()
        res.append((xm.cpu(), loss.clone(), tr.flat_p.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]) and bool(torch.isfinite(res[0][1]))
    assert torch.equal(res[0][2], res[1][2])


@pytest.mark.parametrize("native", [True, False])
def test_meters_on_mixed_steps_count_the_dominant_label(native):
    """(d) DeviceMeters fed by the mixed step -- inside the loss kernels on the native path, by meters.update on the module path --
    equal the restatement applied to each step's logits, its dominant labels and its loss"""
    from mnasnet_pytorch_amd import MixCrossEntropyLoss
    from mnasnet_pytorch_amd.metrics import DeviceMeters, MultiLabelMeters
    from mnasnet_pytorch_amd.train_step import Trainer
    xs = [C.det_input((8, 3, 64, 64), seed=C.INPUT_SEED + i).cuda() for i in range(2)]
    t = _mixed(8)
    meters = DeviceMeters((1, 5))
    m = _model()
    tr = Trainer(m, lr=1e-3, criterion=MixCrossEntropyLoss(0.1), meters=meters)
    tr.native_step = native
    assert (tr._native_head() is not None) == native
    logits = []
    hook = m.register_forward_hook(lambda mod, inp, o: logits.append(o.detach().clone()))
    log = MR.StepLog((1, 5))
    dom = R.dominant(t.a, t.b, t.lam)
    assert torch.equal(dom, t.dominant())
    for x in xs:
        loss = tr.step(x, t)
        z = tr.last_logits if native else logits[-1]
        log.update(z.cpu().numpy(), dom.cpu().numpy(), loss.item())
    hook.remove()
    rec = meters.read()
    print(native, rec)
    log.check(rec)
    assert rec.steps == 2 and rec.samples == 16
    with pytest.raises(ValueError):
        Trainer(m, lr=1e-3, criterion=MixCrossEntropyLoss(0.1), meters=MultiLabelMeters())


def test_validate_runs_the_native_eval_head_with_the_smoothed_loss():
    """(e) validate() under MixCrossEntropyLoss(0.1): the native eval head and the soft loss entry; counts those of a hand-written
    loop, the loss meter within test_cross_entropy's bound of F.cross_entropy(label_smoothing=0.1) per batch"""
    from mnasnet_pytorch_amd import MixCrossEntropyLoss
    from mnasnet_pytorch_amd.train_step import Trainer
    torch.manual_seed(3)
    m = _model()
    tr = Trainer(m, lr=1e-3, criterion=MixCrossEntropyLoss(0.1))
    assert tr._native_eval_head() is not None
    batches = [(C.det_input((8, 3, H, W), seed=C.INPUT_SEED + 40 + i).cuda(), ((torch.arange(8) * 7 + i) % 10).cuda())
               for i, (H, W) in enumerate([(64, 64), (64, 96)])]
    log = MR.StepLog((1, 5))
    m.eval()
    with torch.no_grad():
        for x, t in batches:
            out = m(x)
            log.update(out.cpu().numpy(), t.cpu().numpy(), F.cross_entropy(out, t, label_smoothing=0.1).item())
    m.train()
    lib = tr._native_eval_head().lib
    calls = []
    typed = lib.mnas_head_cross_entropy_soft
    lib.mnas_head_cross_entropy_soft = lambda *a: (calls.append(1), typed(*a))[1]
    try:
        rec = tr.validate(batches)
    finally:
        lib.mnas_head_cross_entropy_soft = typed
    print("validate:", rec, "| hand loop loss avg %.9g" % log.loss.avg)
    assert len(calls) == 2
    assert rec.correct == log.correct and (rec.samples, rec.steps) == (16, 2)
    assert abs(rec.loss.avg - log.loss.avg) <= 2e-5 * max(1.0, abs(log.loss.avg))
    assert abs(rec.loss.val - log.loss.val) <= 2e-5 * max(1.0, abs(log.loss.val))
    assert m.training
