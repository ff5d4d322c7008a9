"""-m gpu: mnas_mlabel_loss / losses.MultiLabelLoss (include/mnas.h "multi-label loss"; csrc/mnas_mlabel.hip).  Identity with
mnas_mlabel_bce when everything is off, the shapes where the row kernel can go wrong (guarded outputs, both paths, both reductions),
per-element brackets (bounds_mlabel_ex.py) on every input kind, torch's BCE-with-logits on the device, mixed label rows and their
meters, bad rows, determinism, graph capture and the module form."""
import ctypes

import numpy as np
import pytest
import torch

import bounds_mlabel as BM
import bounds_mlabel_ex as B
import intervals as IV
import mlabel_ex_ref as X
import multilabel_ref as R
from gpu_util import bits_equal, guarded, relerr
from mnasnet_pytorch_amd import MixedLabels, MultiLabelLoss, MultiLabelMeters
from mnasnet_pytorch_amd import _lib as L
from mnasnet_pytorch_amd.losses import multilabel_loss

pytestmark = pytest.mark.gpu
DICE_TOL = 4 * 2.0 ** -24
OFF = (0.0, 0.0, 0.0, 0.0)


class _Call:
    """one call of mnas_mlabel_loss into canary-guarded dlogits, loss and scratch.  mis = "w" / "pw" / "y" / "dl": that pointer alone
    starts 4 bytes past a 16-byte boundary (any one of them sends a vector-eligible shape down the scalar path)."""

    def __init__(self, z, Y, cfg=OFF, w=None, pw=None, partner=None, lam=None, reduction="mean", meters=None, nw=(0, 0, 0), grad=True,
                 mis=None):
        lib = L.load()
        N, Cn = z.shape
        self.N, self.Cn, self.grad = N, Cn, grad
        self.dl, self.dl_check = guarded((N, Cn), torch.float32, offset=1 if mis == "dl" else 0)
        self.loss_t, self.loss_check = guarded((1,), torch.float32)
        self.nb = int(lib.mnas_mlabel_scratch_bytes(N))
        self.scratch, self.scratch_check = guarded((self.nb // 4,), torch.float32)
        self.keep = []

        def place(x, off):
            buf = torch.zeros(x.numel() + 8, device="cuda")
            buf[off:off + x.numel()] = x.reshape(-1)
            self.keep.append(buf)
            assert (buf.data_ptr() + 4 * off) % 16 == 4 * off
            return buf.data_ptr() + 4 * off
        yptr = place(Y, 1) if mis == "y" else Y.data_ptr()
        wptr = 0 if w is None else place(w, 1 if mis == "w" else 0)
        pptr = 0 if pw is None else place(pw, 1 if mis == "pw" else 0)
        assert z.data_ptr() % 16 == 0 and Y.data_ptr() % 16 == 0 and self.dl.data_ptr() % 16 == (4 if mis == "dl" else 0)
        c = L.MnasMlabelLoss(cfg[0], cfg[1], cfg[2], cfg[3], {"mean": L.MLABEL_MEAN, "rows": L.MLABEL_ROWS}[reduction])
        L.check(lib.mnas_mlabel_loss(z.data_ptr(), yptr, L.ptr(partner), L.ptr(lam), wptr, pptr, N, Cn, ctypes.byref(c),
                                     self.scratch.data_ptr(), self.loss_t.data_ptr(), self.dl.data_ptr() if grad else 0,
                                     meters.kernel_args(z.device) if meters else 0, nw[0], nw[1], nw[2], L.cur_stream()), "mlabel_loss")
        self.loss = self.loss_t[0]

    @property
    def rows(self):
        return self.scratch[2 * self.N:3 * self.N]                 # float loss_rows[N] at byte 8 N

    def ok(self):
        self.dl_check("dlogits", written=self.grad)
        self.loss_check("loss")
        self.scratch_check("scratch", written=False)
        if not self.grad:
            assert bool((self.dl.view(torch.int32) == 0x7FA5A5A5).all()), "forward only wrote into dlogits"
        return self


def _batch(N, Cn, seed=0, **kw):
    return tuple(t.cuda() for t in X.batch(N, Cn, seed, **kw))


# ---- identity with mnas_mlabel_bce ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cn", [(3, 5), (7, 65), (2, 1000), (3, 1024)])
def test_everything_off_is_mlabel_bce_bit_for_bit(N, Cn):
    """gamma = 0, m = 0, eps = 0, no pos_weight, no partner, "mean": loss, gradient, scratch and meters block of
    mnas_mlabel_bce(focal = 0), with and without weights, with a gradient and forward only"""
    from test_gpu_multilabel import _Bce
    z, Y, w, _, _, _ = _batch(N, Cn)
    for wv in (None, w):
        for grad in (True, False):
            ma, mb = MultiLabelMeters(), MultiLabelMeters()
            old = _Bce(z, Y, wv, meters=ma, nw=(N, N, 3), grad=grad)
            new = _Call(z, Y, OFF, wv, meters=mb, nw=(N, N, 3), grad=grad)
            torch.cuda.synchronize()
            old.ok(), new.ok()
            bits_equal(new.loss, old.loss, "loss")
            if grad:
                bits_equal(new.dl, old.dl, "dlogits")
            assert torch.equal(ma.block, mb.block)
            # the scratch: f1_rows, loss_rows and the counts, byte for byte; `scale` is written by neither
            from test_gpu_multilabel import G
            assert torch.equal(old.scratch[G:G + 24 * N], new.scratch.view(torch.uint8)[:24 * N])
            assert bool((old.scratch[G + 24 * N:G + old.nb] == 0xA5).all())
            assert bool((new.scratch.view(torch.int32)[6 * N:] == 0x7FA5A5A5).all())


# ---- shapes where the row kernel can go wrong ---------------------------------------------------------------------------------------
def _check_against_rule(call, ref, what):
    loss, g = ref
    got = float(call.loss)
    assert abs(got - loss) <= 2e-5 * abs(loss), (what, got, loss)
    gerr = relerr(call.dl.cpu(), torch.from_numpy(g))
    assert gerr < 1e-5, (what, gerr)


@pytest.mark.parametrize("N,Cn", B.EX_SHAPES)
def test_shapes(N, Cn):
    """one class; a partial wave; one lane either side of a wave; one past the workgroup's stride with C % 4 != 0; the 16-byte path
    and its second trip; N past the batch stage's stride.  Canary-guarded outputs; weights, pos_weight and labels each once 4 bytes
    off alignment (the scalar path; dlogits bit-equal to the aligned run: every element is computed alone); forward only and with
    meters give the same loss bits; four configurations, both reductions, against the fp64 rule."""
    z, Y, w, pw, _, _ = _batch(N, Cn)
    zn, Yn, wn, pn = (t.cpu().numpy() for t in (z, Y, w, pw))
    f1, counts, dice = R.f1_batch(zn, Yn), R.dice_counts(zn, Yn), R.hard_dice(zn, Yn)
    for cfg in B.EX_CONFIGS:
        pwv = pw if cfg[4] else None
        for red in ("mean", "rows"):
            ref = X.loss_and_grad(zn, Yn, wn, pn if cfg[4] else None, *cfg[:4], reduction=red)[:2]
            m = MultiLabelMeters()
            base = _Call(z, Y, cfg[:4], w, pwv, reduction=red)
            fwd = _Call(z, Y, cfg[:4], w, pwv, reduction=red, grad=False)
            met = _Call(z, Y, cfg[:4], w, pwv, reduction=red, meters=m, nw=(N, N, 3))
            others = [_Call(z, Y, cfg[:4], w, pwv, reduction=red, mis=mis) for mis in ("w", "y") + (("pw",) if cfg[4] else ())]
            torch.cuda.synchronize()
            for c in [base, fwd, met] + others:
                c.ok()
            _check_against_rule(base, ref, (cfg, red))
            bits_equal(fwd.loss, base.loss, "forward-only loss")
            bits_equal(met.loss, base.loss, "loss with meters")
            bits_equal(met.dl, base.dl, "dlogits with meters")
            for c in others:
                bits_equal(c.dl, base.dl, "dlogits on the scalar path")
                assert abs(float(c.loss) - ref[0]) <= 2e-5 * abs(ref[0])
            rec = m.read()
            assert rec.f1.val == f1 and (rec.last_tp, rec.last_fp, rec.last_fn) == counts and abs(rec.hdice.val - dice) <= DICE_TOL
            assert (rec.steps, rec.samples, rec.loss_n, rec.hdice_n, rec.f1_n) == (1, N, N, N, 3)
            assert rec.loss.val == float(base.loss)


# ---- accuracy: per-element brackets ------------------------------------------------------------------------------------------------
def _check_bounds(call, z, Y, w, pw, cfg, vec, what, partner=None, lam=None, reduction="mean"):
    N, Cn = z.shape
    iv = B.mlabel_ex_intervals(z, Y, w, pw, N, Cn, cfg, vec, partner, lam, reduction, rows_dev=call.rows)
    r1 = IV.check_interval(call.dl, iv["dl"], what + " dlogits", "mlabel_ex dlogits")
    r2 = B.check_rows(call.rows, iv, what)
    IV.WORST["mlabel_ex rows"] = max(IV.WORST.get("mlabel_ex rows", 0.0), r2)
    r3 = IV.check_interval(call.loss.reshape(()), iv["loss"], what + " loss", "mlabel_ex loss")
    return r1, r2, r3, iv


@pytest.mark.parametrize("kind", BM.ML_KINDS)
def test_bounds(kind):
    """every gradient element, every row sum and the loss inside their brackets, on every input kind (|z| up to 200; soft labels;
    power-of-two and zero weights; one live weight per row, which the row bound must still see), for the four configurations,
    plain and with mixed rows, on a scalar-path and a vector-path shape"""
    worst = [0.0, 0.0, 0.0]
    for (N, Cn) in ((5, 257), (3, 1024)):
        z, Y, w = (t.cuda() for t in BM.mlabel_inputs(kind, N, Cn))
        _, _, _, pw, partner, lam = _batch(N, Cn)
        for cfg in B.EX_CONFIGS:
            pwv = pw if cfg[4] else None
            for pa, la in ((None, None), (partner, lam)):
                red = "rows" if pa is not None else "mean"
                call = _Call(z, Y, cfg[:4], w, pwv, pa, la, reduction=red).ok()
                r = _check_bounds(call, z, Y, w, pwv, cfg[:4], Cn % 4 == 0, "%s %s %s" % (kind, (N, Cn), cfg), pa, la, red)
                worst = [max(a, b) for a, b in zip(worst, r[:3])]
                if kind == "sparse" and pa is None and cfg[2] == 0.0:      # (beyond a margin a live element's loss is exactly 0)
                    BM.mlabel_probe_visible(r[3], BM.mlabel_live(N, Cn), kind)
    print("mlabel_ex %s: worst error / bracket: dlogits %.3f, rows %.3f, loss %.3f" % (kind, worst[0], worst[1], worst[2]))


# ---- against torch on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", R.GRID_C)
def test_against_torch_bce_with_logits(Cn):
    """gamma = 0, m = 0 with pos_weight and weights against fp32 F.binary_cross_entropy_with_logits on the device, within
    test_gpu_multilabel.py::test_grid_loss_and_gradient's bounds: 2e-5 for the loss, 1e-5 for the gradient"""
    N = R.GRID_N
    z, Y, w, pw, _, _ = _batch(N, Cn, seed=1)
    zr = z.clone().requires_grad_(True)
    want = torch.nn.functional.binary_cross_entropy_with_logits(zr, Y, weight=w, pos_weight=pw)
    want.backward()
    call = _Call(z, Y, OFF, w, pw).ok()
    want = want.detach()
    err = abs(float(call.loss) - float(want)) / abs(float(want))
    gerr = relerr(call.dl, zr.grad)
    print("C %d: loss error to torch %.3g (bound 2e-5), gradient %.3g (bound 1e-5)" % (Cn, err, gerr))
    assert err <= 2e-5 and gerr < 1e-5


# ---- mixed labels -----------------------------------------------------------------------------------------------------------------------
def _mix_cases(N):
    ar = torch.arange(N)
    yield "lam 0", ar.roll(1), torch.zeros(N)
    yield "lam 1", ar.roll(1), torch.ones(N)
    yield "lam 0.5", ar.roll(1), torch.full((N,), 0.5)
    yield "partner n", ar, torch.linspace(0.1, 0.9, N)
    g = torch.Generator().manual_seed(5)
    yield "permutation", torch.randperm(N, generator=g), torch.rand(N, generator=g)


@pytest.mark.parametrize("cfg", [B.EX_CONFIGS[2], (0.0, 0.0, 0.0, 0.1, False)])
def test_mixed_labels_equal_the_dense_call_and_count_the_dominant_image(cfg):
    """a MixedLabels call against the same call on .dense(): each inside the other's bracket (the dense call's labels are exact data,
    the mixed call's carry the mixing's two roundings); the meters count the dominant image's raw labels"""
    N, Cn = 6, 257
    z, Y, w, pw, _, _ = _batch(N, Cn, seed=2)
    pwv = pw if cfg[4] else None
    for name, partner, lam in _mix_cases(N):
        partner, lam = partner.cuda(), lam.cuda()
        ml = MixedLabels(Y, partner, lam)
        m = MultiLabelMeters()
        mixed = _Call(z, Y, cfg[:4], w, pwv, partner, lam, meters=m, nw=(N, N, 3)).ok()
        dense = _Call(z, ml.dense().contiguous(), cfg[:4], w, pwv).ok()
        ivm = B.mlabel_ex_intervals(z, Y, w, pwv, N, Cn, cfg[:4], False, partner, lam)
        # the dense labels lie inside the mixed labels' bracket (torch rounds lam*Y, (1-lam)*Y[p] and the sum: one rounding more)
        t_d = B.label_intervals(ml.dense(), None, None, cfg[3])
        slack = 2.0 ** -23 * ivm["t"].amax + IV.TINY32
        assert bool((t_d.lo >= ivm["t"].lo - slack).all()) and bool((t_d.hi <= ivm["t"].hi + slack).all()), name
        IV.check_interval(mixed.dl, ivm["dl"], name + " mixed dlogits", "mlabel_ex dlogits")
        ivd = B.mlabel_ex_intervals(z, ml.dense().contiguous(), w, pwv, N, Cn, cfg[:4], False)
        IV.check_interval(dense.dl, ivd["dl"], name + " dense dlogits", "mlabel_ex dlogits")
        ref = X.loss_and_grad(z.cpu().numpy(), Y.cpu().numpy(), w.cpu().numpy(), None if pwv is None else pw.cpu().numpy(), *cfg[:4],
                              partner=partner.cpu().numpy(), lam=lam.cpu().numpy())[:2]
        _check_against_rule(mixed, ref, name)
        _check_against_rule(dense, ref, name + " dense")
        if name in ("lam 1",):                               # y = Y exactly: the mixed call is the plain call, bit for bit
            plain = _Call(z, Y, cfg[:4], w, pwv).ok()
            bits_equal(mixed.dl, plain.dl, "lam 1 dlogits")
            bits_equal(mixed.loss, plain.loss, "lam 1 loss")
        dom = ml.dominant().cpu().numpy()
        assert np.array_equal(dom, X.dominant(Y.cpu().numpy(), partner.cpu().numpy(), lam.cpu().numpy()))
        zn = z.cpu().numpy()
        rec = m.read()
        assert rec.f1.val == R.f1_batch(zn, dom), name
        assert (rec.tp, rec.fp, rec.fn) == R.dice_counts(zn, dom), name
        assert abs(rec.hdice.val - R.hard_dice(zn, dom)) <= DICE_TOL, name


@pytest.mark.parametrize("what,partner_v,lam_v", [("partner = N", None, 0.3), ("partner = -1", -1, 0.3), ("lam = NaN", 1, float("nan")),
                                                  ("lam = 1.5", 1, 1.5)])
def test_bad_row(what, partner_v, lam_v):
    """a row whose partner lies outside [0, N) or whose weight lies outside [0, 1]: NaN loss, NaN gradient row, every other row as
    in a run without it, canaries intact, nonfinite_steps bumped (the kernel reads no partner row for such a row)"""
    N, Cn = 5, 1024
    z, Y, w, pw, partner, lam = _batch(N, Cn, seed=4)
    cfg = B.EX_CONFIGS[2]
    good = _Call(z, Y, cfg[:4], w, pw, partner, lam).ok()
    p2, l2 = partner.clone(), lam.clone()
    p2[2] = N if partner_v is None else partner_v
    l2[2] = lam_v
    m = MultiLabelMeters()
    bad = _Call(z, Y, cfg[:4], w, pw, p2, l2, meters=m, nw=(N, N, 3))
    torch.cuda.synchronize()
    bad.ok()
    assert bool(torch.isnan(bad.loss)) and bool(torch.isnan(bad.dl[2]).all()) and bool(torch.isnan(bad.rows[2]))
    keep = [0, 1, 3, 4]
    bits_equal(bad.dl[keep], good.dl[keep], "the other rows")
    bits_equal(bad.rows[keep], good.rows[keep], "the other row sums")
    rec = m.read()
    assert rec.nonfinite_steps == 1 and rec.steps == 1


# ---- determinism, capture, module form --------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    N, Cn = 257, 1000
    z, Y, w, pw, partner, lam = _batch(N, Cn, seed=6)
    a = _Call(z, Y, B.EX_CONFIGS[2][:4], w, pw, partner, lam, reduction="rows").ok()
    b = _Call(z, Y, B.EX_CONFIGS[2][:4], w, pw, partner, lam, reduction="rows").ok()
    bits_equal(a.loss, b.loss, "loss")
    bits_equal(a.dl, b.dl, "dlogits")
    bits_equal(a.rows, b.rows, "row sums")


def test_call_is_capturable_in_a_graph():
    """a linear single-stream capture of one fused call: three replays move the block three times and leave the eager call's bits"""
    N, Cn = 12, 1000
    z, Y, w, pw, partner, lam = _batch(N, Cn, seed=7)
    m = MultiLabelMeters()
    kw = dict(gamma_pos=1.0, gamma_neg=4.0, margin=0.05, label_smoothing=0.1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = multilabel_loss(z, Y, partner, lam, w, pw, meters=m, meter_weights=(N, N, 3), **kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    m.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        loss, dl = multilabel_loss(z, Y, partner, lam, w, pw, meters=m, meter_weights=(N, N, 3), **kw)
    for _ in range(3):
        graph.replay()
    rec = m.read()
    assert (rec.steps, rec.samples, rec.loss_n, rec.f1_n) == (3, 3 * N, 3 * N, 9)
    bits_equal(loss, eager[0], "replayed loss")
    bits_equal(dl, eager[1], "replayed dlogits")
    dom = MixedLabels(Y, partner, lam).dominant().cpu().numpy()
    tp, fp, fn = R.dice_counts(z.cpu().numpy(), dom)
    assert (rec.tp, rec.fp, rec.fn) == (3 * tp, 3 * fp, 3 * fn)


def test_module_form():
    """MultiLabelLoss as an nn.Module: the loss of the raw entry, d loss / d outputs = dlogits * grad_output bitwise, weights
    ignored unless use_weight_mask, forward only without requires_grad, integer label matrices converted with .float(), a
    MixedLabels target, pos_weight moved with the module"""
    N, Cn = 12, 90
    z, Y, w, pw, partner, lam = _batch(N, Cn, seed=8)
    for weighted in (False, True):
        for target, pa, la in ((Y, None, None), (MixedLabels(Y, partner, lam), partner, lam)):
            raw = _Call(z, Y, (1.0, 4.0, 0.05, 0.1), w if weighted else None, pw, pa, la, reduction="rows").ok()
            crit = MultiLabelLoss(1, 4, 0.05, pos_weight=pw.cpu(), label_smoothing=0.1, use_weight_mask=weighted, reduction="rows").cuda()
            assert crit.pos_weight.device.type == "cuda"
            zr = z.clone().requires_grad_(True)
            loss = crit(zr, target, w)
            (loss * 3.0).backward()
            bits_equal(loss.detach(), raw.loss, "module loss")
            bits_equal(zr.grad, raw.dl * 3.0, "module gradient")
            with torch.no_grad():
                bits_equal(crit(z, target, w), raw.loss, "forward only")
    crit = MultiLabelLoss(2, 2)
    bits_equal(crit(z, Y.long()), crit(z, Y), "integer labels")
    with pytest.raises(ValueError):
        crit(z, Y[:, :5])
    with pytest.raises(ValueError):
        MultiLabelLoss(pos_weight=torch.ones(3)).cuda()(z, Y)
