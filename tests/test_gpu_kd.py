"""-m gpu: class weights and knowledge distillation in the cross-entropy kernels (csrc/mnas_head.hip: k_head_ce_kd,
k_head_loss_mean_kd) through the C ABI: against the fp64 restatement (tests/kd_ref.py), inside the per-element brackets of
tests/bounds_kd.py, the edge rules of include/mnas.h one by one, consistency with the plain and soft kernels, determinism, meters."""
import functools

import pytest
import torch

import bounds_kd as BK
import bounds_tail as BT
import gpu_util as G
import intervals as IV
import kd_ref as K
from gpu_util import relerr
from mnasnet_pytorch_amd import _lib as L

pytestmark = pytest.mark.gpu

# student rows of every kind of bounds_tail.ce_logits asked for; the odd positions are the mixed batches (_inputs).  peak_on sits at one:
# a batch of plain labels whose EVERY row is saturated on its label has a gradient of 1e-15 all over, which no fp32 softmax resolves
# (p rounds to 1, as in k_head_ce), so a tolerance relative to the largest element says nothing there -- that batch is held to
# the per-element bracket alone (test_kd_per_element_bracket), like teacher == student
KINDS = ["uniform4", "peak_on", "uniform40", "peak_off", "equal", "plus1000"]
# (N, C, T, alpha, eps, weights): every value of the grid occurs; C = 257 and N = 300 each meet alpha 0, 0.5 and 1
GRID = [(1, 1, 1.0, 0.5, 0.0, "none"), (3, 2, 2.0, 0.0, 0.1, "positive"), (3, 5, 4.5, 1.0, 0.1, "zeros"),
        (37, 255, 2.0, 0.5, 0.1, "positive"), (37, 256, 1.0, 1.0, 0.0, "zeros"), (37, 257, 2.0, 0.0, 0.1, "zeros"),
        (3, 257, 4.5, 0.5, 0.0, "positive"), (37, 257, 1.0, 1.0, 0.1, "none"), (300, 5, 2.0, 0.0, 0.0, "none"),
        (300, 257, 4.5, 0.5, 0.1, "zeros"), (300, 2, 1.0, 1.0, 0.1, "positive"), (37, 1003, 2.0, 0.5, 0.1, "positive")]
LAM = torch.tensor([0.0, 0.5, 1.0, 0.3, 0.8125, 0.49999997])


def _weights(Cn, how):
    if how == "none":
        return None
    w = torch.rand(Cn, generator=torch.Generator().manual_seed(3)) + 0.25
    if how == "zeros":
        w[1::3] = 0.0
    return w


def _dev(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _inputs(N, Cn, i, kind):
    """run i of a grid case: student rows of `kind`, teacher rows of another kind, every second run a mixed batch, rows ignored in
    two of three"""
    z = BT.ce_logits(kind, N, Cn)
    t = BT.ce_logits(KINDS[(i + 2) % len(KINDS)], N, Cn, seed=29)
    a, b = BT.ce_targets(N, Cn)
    if N > 1 and i % 3 != 0:
        a = BT.ce_ignore(a, "third")
    lam = LAM[torch.arange(N) % 6].clone()
    return (z, t, a) + ((b, lam) if i % 2 == 1 else (None, None))


@functools.lru_cache(maxsize=None)
def _runs(case):
    """the launches of one grid case, made once and shared by the tests that read them: [(inputs, host outputs)]"""
    N, Cn, T, alpha, eps, how = case
    w = _weights(Cn, how)
    kd = BK.KD(N, Cn)
    out = []
    for i, kind in enumerate(KINDS):
        z, t, a, b, lam = _inputs(N, Cn, i, kind)
        what = "kd %s run %d (%s)" % (case, i, kind)
        res = kd.run(*_dev(z, a, b, lam), eps, *_dev(w, t), T, alpha, what=what)
        out.append(((z, t, a, b, lam, w), res, what))
    return out


@pytest.mark.parametrize("case", GRID)
def test_kd_against_fp64(case):
    """the loss and both parts within 2e-5 max(1, |ref|) of kd_ref, dlogits at relerr < 1e-5 (the tolerances of
    test_gpu_mix.py::test_soft_cross_entropy_against_fp64)"""
    N, Cn, T, alpha, eps, how = case
    for (z, t, a, b, lam, w), res, what in _runs(case):
        ref = K.kd_loss(z, a, b, lam, eps, w, t, T, alpha)
        assert res["bad"] == 0 and not bool(torch.isnan(res["dl"]).any()), what
        got = dict(loss=float(res["loss"]), hard=float(res["parts"][0]), kd=float(res["parts"][1]))
        print("%s  loss %.8f ref %.8f  hard %.8f ref %.8f  kd %.8f ref %.8f  relerr(dlogits) %.2e"
              % (what, got["loss"], float(ref["loss"]), got["hard"], float(ref["hard"]), got["kd"], float(ref["kd"]),
                 relerr(res["dl"], ref["grad"])))
        for k, v in got.items():
            assert abs(v - float(ref[k])) < 2e-5 * max(1.0, abs(float(ref[k]))), (what, k, v, float(ref[k]))
        assert relerr(res["dl"], ref["grad"]) < 1e-5, what


@pytest.mark.parametrize("case", GRID)
def test_kd_per_element_bracket(case):
    """EVERY dlogits element, both halves of loss_rows and the two means (and the total) inside bounds_kd.kd_intervals; the case
    teacher == student (kd = 0 by cancellation) as well; a dlogits element scaled by 1.001 and a kd mean formed with T instead of
    T^2 are rejected by the same checker"""
    N, Cn, T, alpha, eps, how = case
    worst, rejected = 0.0, 0
    for (z, t, a, b, lam, w), res, what in _runs(case):
        iv = BK.kd_intervals(z, a, b, lam, eps, w, t, T, alpha)
        worst = max(worst, BK.check_kd(res["dl"], res["rows"], res["parts"], res["loss"], iv, what))
        # the checker must catch a corrupted result
        dl = res["dl"].clone()
        k = int(dl.abs().argmax())
        if float(dl.view(-1)[k]) != 0.0:
            dl.view(-1)[k] *= 1.001
            with pytest.raises(AssertionError):
                BK.check_kd(dl, res["rows"], res["parts"], res["loss"], iv, what, family=None)
            rejected += 1
        if iv["kd"] and T != 1.0 and abs(float(res["parts"][1])) > 1e-3:
            parts = res["parts"].clone()
            parts[1] = torch.tensor(T, dtype=torch.float32) * (res["rows"][N:].sum() / N)
            with pytest.raises(AssertionError):
                BK.check_kd(res["dl"], res["rows"], parts, res["loss"], iv, what, family=None)
            rejected += 2
    # teacher == student: nothing to compare relatively; the bracket holds and the value is a rounding residue.  Once on a mixed
    # batch, once on plain labels with every row saturated on its label (the gradient is a residue as well)
    w = _weights(Cn, how)
    for i, kind in ((1, "uniform4"), (0, "peak_on")):
        z, _, a, b, lam = _inputs(N, Cn, i, kind)
        res = BK.KD(N, Cn).run(*_dev(z, a, b, lam), eps, *_dev(w, z.clone()), T, alpha, what="t == z")
        iv = BK.kd_intervals(z, a, b, lam, eps, w, z.clone(), T, alpha)
        worst = max(worst, BK.check_kd(res["dl"], res["rows"], res["parts"], res["loss"], iv, "kd %s t == z, %s" % (case, kind)))
        assert abs(float(res["parts"][1])) < 1e-5
    print("distillation cross-entropy %s: worst error / bracket %.3f, %d corrupted results rejected" % (case, worst, rejected),
          {k: round(v, 4) for k, v in IV.WORST.items() if "distillation" in k})
    assert worst <= 1.0
    assert rejected >= (1 if Cn > 1 else 0)
    if alpha != 0.0 and T != 1.0 and Cn > 1:
        assert rejected >= 3


# ---- the edge rules of include/mnas.h "distillation cross-entropy", one assertion each ------------------------------------------------
def _edge(N=5, Cn=7):
    z, t = BT.ce_logits("uniform4", N, Cn), BT.ce_logits("uniform4", N, Cn, seed=31)
    a, b = BT.ce_targets(N, Cn)
    return z, t, a, b, LAM[torch.arange(N) % 6].clone(), _weights(Cn, "positive")


def test_masked_teacher_classes_give_a_finite_loss():
    z, t, a, b, lam, w = _edge()
    t[:, 1] = float("-inf")
    t[0, 2] = float("-inf")
    res = BK.KD(5, 7).run(*_dev(z, a, b, lam), 0.1, *_dev(w, t), 2.0, 0.5)
    ref = K.kd_loss(z, a, b, lam, 0.1, w, t, 2.0, 0.5)
    assert bool(torch.isfinite(res["rows"]).all()) and bool(torch.isfinite(res["dl"]).all()) and bool(torch.isfinite(res["loss"]))
    assert abs(float(res["loss"]) - float(ref["loss"])) < 2e-5 * max(1.0, abs(float(ref["loss"])))
    assert abs(float(res["parts"][1]) - float(ref["kd"])) < 2e-5 * max(1.0, abs(float(ref["kd"])))
    assert relerr(res["dl"], ref["grad"]) < 1e-5


def test_masked_student_class_under_teacher_mass_gives_an_infinite_row_and_a_finite_gradient():
    z, t, a, b, lam, w = _edge()
    a[1], b[1] = 0, 2
    z[1, 3] = float("-inf")                                   # no label of row 1, but the teacher puts mass there
    res = BK.KD(5, 7).run(*_dev(z, a, b, lam), 0.0, *_dev(w, t), 2.0, 0.5)
    rows = res["rows"]
    assert float(rows[5 + 1]) == float("inf") and bool(torch.isfinite(rows[5:][[0, 2, 3, 4]]).all())
    assert bool(torch.isfinite(rows[:5]).all())               # eps == 0: the hard row stays finite
    assert float(res["parts"][1]) == float("inf") and float(res["loss"]) == float("inf")
    assert bool(torch.isfinite(res["dl"]).all())
    assert relerr(res["dl"], K.kd_loss(z, a, b, lam, 0.0, w, t, 2.0, 0.5)["grad"]) < 1e-5


def test_alpha_one_leaves_an_infinite_hard_row_out():
    z, t, a, b, lam, w = _edge()
    a[1], b[1] = 0, 2
    z[1, 3] = t[1, 3] = float("-inf")                         # masked for both: +inf hard row under smoothing, finite kd
    res = BK.KD(5, 7).run(*_dev(z, a, b, lam), 0.1, *_dev(w, t), 2.0, 1.0)
    assert float(res["rows"][1]) == float("inf") and float(res["parts"][0]) == float("inf")
    assert bool(torch.isfinite(res["rows"][5:]).all()) and bool(torch.isfinite(res["loss"]))
    assert float(res["loss"]) == float(res["parts"][1])
    assert bool(torch.isfinite(res["dl"]).all())
    ref = K.kd_loss(z, a, b, lam, 0.1, w, t, 2.0, 1.0)
    assert abs(float(res["loss"]) - float(ref["kd"])) < 2e-5 * max(1.0, abs(float(ref["kd"]))) and relerr(res["dl"], ref["grad"]) < 1e-5
    half = BK.KD(5, 7).run(*_dev(z, a, b, lam), 0.1, *_dev(w, t), 2.0, 0.5)
    assert float(half["loss"]) == float("inf")                # any other alpha keeps the hard term


def test_ignored_rows_leave_the_hard_term_and_stay_in_the_distillation_term():
    z, t, a, b, lam, w = _edge()
    a[1], b[3] = -100, -100
    kd = BK.KD(5, 7)
    res = kd.run(*_dev(z, a, b, lam), 0.1, *_dev(w, t), 2.0, 0.5)
    ref = K.kd_loss(z, a, b, lam, 0.1, w, t, 2.0, 0.5)
    assert res["bad"] == 0 and float(res["rows"][1]) == 0.0 and float(res["rows"][3]) == 0.0
    assert bool((res["rows"][5:] > 0).all())
    assert relerr(res["dl"][[1, 3]], ref["grad"][[1, 3]]) < 1e-5 and bool((res["dl"][[1, 3]] != 0).any())
    assert abs(float(res["loss"]) - float(ref["loss"])) < 2e-5 * max(1.0, abs(float(ref["loss"])))
    hard_only = kd.run(*_dev(z, a, b, lam), 0.1, *_dev(w, None), 2.0, 0.5)
    assert bool((hard_only["dl"][[1, 3]] == 0).all()) and bool((hard_only["rows"][5:] == 0).all())
    assert float(hard_only["loss"]) == float(hard_only["parts"][0]) and float(hard_only["parts"][1]) == 0.0
    assert abs(float(hard_only["loss"]) - float(ref["hard"])) < 2e-5 * max(1.0, abs(float(ref["hard"])))


def test_all_rows_ignored():
    z, t, a, b, lam, w = _edge()
    none = torch.full((5,), -100)
    kd = BK.KD(5, 7)
    for alpha in (0.5, 1.0):
        res = kd.run(*_dev(z, none, None, None), 0.1, *_dev(w, t), 2.0, alpha)
        ref = K.kd_loss(z, none, None, None, 0.1, w, t, 2.0, alpha)
        assert bool(torch.isnan(res["parts"][0])) and bool(torch.isfinite(res["parts"][1])), alpha
        assert abs(float(res["parts"][1]) - float(ref["kd"])) < 2e-5 * max(1.0, abs(float(ref["kd"])))
        assert bool(torch.isnan(res["loss"])) == (alpha != 1.0), alpha
        assert bool((res["rows"][:5] == 0).all()) and relerr(res["dl"], ref["grad"]) < 1e-5
    res = kd.run(*_dev(z, none, None, None), 0.1, *_dev(w, t), 2.0, 0.0)
    assert bool(torch.isnan(res["loss"])) and bool((res["dl"] == 0).all())


@pytest.mark.parametrize("N,Cn", [(7, 10), (33, 257)])
def test_refused_labels_and_weights(N, Cn):
    """the bad flag is set, the loss and both parts are NaN, the refused row's gradient is zero, nothing outside the outputs is
    written (BK.KD.run checks the canaries around every output buffer)"""
    z, t = BT.ce_logits("uniform4", N, Cn), BT.ce_logits("uniform4", N, Cn, seed=31)
    a, b = BT.ce_targets(N, Cn)
    lam, w = torch.full((N,), 0.3), _weights(Cn, "zeros")
    kd = BK.KD(N, Cn)
    ok = kd.run(*_dev(z, a, b, lam), 0.1, *_dev(w, t), 2.0, 0.5)
    assert ok["bad"] == 0 and bool(torch.isfinite(ok["loss"]))
    for what, val in (("a", Cn), ("a", -1), ("a", 2 ** 40), ("b", Cn), ("b", -7), ("lam", 1.5), ("lam", float("nan")), ("lam", -0.25),
                      ("lam", float("inf"))):
        aa, bb, ll = a.clone(), b.clone(), lam.clone()
        {"a": aa, "b": bb, "lam": ll}[what][2] = val
        for alpha in (0.5, 1.0):
            res = kd.run(*_dev(z, aa, bb, ll), 0.1, *_dev(w, t), 2.0, alpha, what="refused %s %r" % (what, val))
            assert res["bad"] == 1 and bool(torch.isnan(res["loss"])) and bool(torch.isnan(res["parts"]).all()), (what, val, alpha)
            assert bool((res["dl"][2] == 0).all()) and not bool(torch.isnan(res["dl"]).any()), (what, val, alpha)
            assert bool(torch.isnan(res["rows"][2])) and bool(torch.isnan(res["rows"][N + 2])), (what, val, alpha)
    aa = a.clone()
    aa[0] = Cn + 5
    res = kd.run(*_dev(z, aa, None, None), 0.1, *_dev(w, None), 2.0, 0.5)          # without mixing and without a teacher as well
    assert res["bad"] == 1 and bool(torch.isnan(res["loss"])) and bool((res["dl"][0] == 0).all())
    aa, bb = a.clone(), b.clone()
    aa[3], bb[3] = -100, Cn                                   # an ignored row hides a refused partner label
    res = kd.run(*_dev(z, aa, bb, lam), 0.1, *_dev(w, t), 2.0, 0.5)
    assert res["bad"] == 0 and bool(torch.isfinite(res["loss"]))


def test_einval_launches_nothing():
    N, Cn = 7, 10
    z, t = BT.ce_logits("uniform4", N, Cn), BT.ce_logits("uniform4", N, Cn, seed=31)
    a, b = BT.ce_targets(N, Cn)
    dev = _dev(z, a, b, torch.full((N,), 0.3))
    w, td = _dev(_weights(Cn, "positive"), t)
    kd = BK.KD(N, Cn)
    kd.fill()
    kd.ranks.fill_(-7)
    fn = L.load().mnas_head_cross_entropy_kd
    good = list(kd.args(*dev, 0.1, w, td, 2.0, 0.5))
    EPS, TEMP, ALPHA, NN, CC = 4, 7, 8, 9, 10
    bad_calls = [(TEMP, 0.0), (TEMP, -1.0), (TEMP, float("nan")), (ALPHA, -0.1), (ALPHA, 1.5), (ALPHA, float("nan")), (EPS, -0.1), (EPS, 1.5),
                 (EPS, float("nan")), (0, 0), (1, 0), (12, 0), (13, 0), (16, 0), (NN, 0), (CC, 0), (NN, -3)]
    for slot, val in bad_calls:
        args = list(good)
        args[slot] = val
        assert fn(*args) == L.EINVAL, (slot, val)
    from mnasnet_pytorch_amd.metrics import DeviceMeters
    meters = DeviceMeters((1, 5))
    args = list(kd.args(*dev, 0.1, w, td, 2.0, 0.5, meters=meters))
    args[19] = 0                                              # meters without rank_rows
    assert fn(*args) == L.EINVAL
    args = list(kd.args(*dev, 0.1, w, td, 2.0, 0.5, meters=meters))
    args[18] = 0                                              # meters with nk = 0
    assert fn(*args) == L.EINVAL
    torch.cuda.synchronize()
    for name in ("dl", "rows", "parts", "loss"):
        assert bool(torch.isnan(getattr(kd, name)).all()), name + " was written by a refused call"
    assert int(kd.bad) == 0 and bool((kd.ranks == -7).all()) and meters.read().steps == 0
    assert fn(*good) == 0                                     # ... and the same arguments unchanged do launch
    torch.cuda.synchronize()
    assert bool(torch.isfinite(kd.loss).all())


# ---- consistency with the existing kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cn", [(7, 255), (37, 257), (3, 1003)])
def test_without_weights_and_teacher_inside_the_soft_kernels_bracket(N, Cn):
    """w = NULL, t = NULL and w == 1.0 given explicitly: dlogits, the hard rows and the loss inside bounds_tail.ce_intervals for the
    same inputs, whatever alpha is"""
    kd = BK.KD(N, Cn)
    ones = torch.ones(Cn)
    worst = 0.0
    for i, kind in enumerate(BT.CE_ROWS):
        z = BT.ce_logits(kind, N, Cn)
        a, b = BT.ce_targets(N, Cn)
        b = torch.where(torch.arange(N) % 4 == 1, a, b)
        a = BT.ce_ignore(a, BT.CE_IGNORE[i % 4])
        lam = LAM[torch.arange(N) % 6].clone()
        for eps in (0.0, 0.1):
            for bb, ll in ((None, None), (b, lam)):
                iv = BT.ce_intervals(z, a, bb, ll, eps)
                for w, alpha in ((None, 0.5), (ones, 0.0), (ones, 1.0)):
                    what = "kd as soft ce %s eps %g mixed %s w %s (%d, %d)" % (kind, eps, bb is not None, w is not None, N, Cn)
                    res = kd.run(*_dev(z, a, bb, ll), eps, *_dev(w, None), 3.0, alpha, what=what)
                    rows = res["rows"][:N]
                    assert res["bad"] == 0 and bool((res["rows"][N:] == 0).all()) and float(res["parts"][1]) == 0.0, what
                    G.bits_equal(res["parts"][0:1], res["loss"].reshape(1), what + " hard part vs loss")
                    assert bool((res["dl"][~iv["valid"]] == 0).all()) and bool((rows[~iv["valid"]] == 0).all()), what
                    r = [IV.check_interval(res["dl"], iv["dl"], what + " dlogits", "distillation as soft cross-entropy"),
                         IV.check_interval(rows, iv["rows"], what + " rows", "distillation as soft cross-entropy"),
                         BT.check_ce_mean(res["loss"], rows, iv["count"], what + " mean", "distillation as soft cross-entropy mean")]
                    worst = max(worst, *r)
    print("distillation kernel without weights and teacher (%d, %d): worst error / soft bracket %.3f" % (N, Cn, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_criterion_without_weight_and_teacher_is_bit_equal_to_mix_cross_entropy(eps):
    from mnasnet_pytorch_amd import DistillCrossEntropyLoss, MixCrossEntropyLoss, MixedTarget
    N, Cn = 37, 257
    z = BT.ce_logits("uniform4", N, Cn).cuda()
    a, b = BT.ce_targets(N, Cn)
    a = BT.ce_ignore(a, "third")
    mixed = MixedTarget(a, b, LAM[torch.arange(N) % 6].clone()).to("cuda")
    for target in (a.cuda(), mixed):
        out = []
        for crit in (DistillCrossEntropyLoss(label_smoothing=eps), MixCrossEntropyLoss(eps)):
            zz = z.clone().requires_grad_(True)
            loss = crit(zz, target)
            loss.backward()
            out.append((loss.detach().clone(), zz.grad.clone()))
        G.bits_equal(out[0][0].reshape(1), out[1][0].reshape(1), "loss")
        G.bits_equal(out[0][1], out[1][1], "gradient")
        assert bool(torch.isfinite(out[0][0]))


def test_criterion_forward_backward_and_parts():
    """the module path: DistillCrossEntropyLoss on a DistillTarget through autograd against kd_ref; last_parts on the device; no
    gradient to the teacher logits; the refused-label flag surfaces in check_targets()"""
    from mnasnet_pytorch_amd import DistillCrossEntropyLoss, DistillTarget, MixedTarget
    N, Cn = 37, 257
    z, t = BT.ce_logits("uniform4", N, Cn), BT.ce_logits("peak_off", N, Cn, seed=31)
    a, b = BT.ce_targets(N, Cn)
    lam, w = LAM[torch.arange(N) % 6].clone(), _weights(Cn, "zeros")
    crit = DistillCrossEntropyLoss(2.0, 0.5, 0.1, weight=w).cuda()
    assert crit.weight.is_cuda and crit.last_parts is None
    td = t.cuda().requires_grad_(True)
    for target, (bb, ll) in ((a.cuda(), (None, None)), (MixedTarget(a, b, lam).to("cuda"), (b, lam))):
        zz = z.cuda().requires_grad_(True)
        loss = crit(zz, DistillTarget(target, td))
        (loss * 3.0).backward()
        ref = K.kd_loss(z, a, bb, ll, 0.1, w, t, 2.0, 0.5)
        assert abs(float(loss.detach()) - float(ref["loss"])) < 2e-5 * max(1.0, abs(float(ref["loss"])))
        assert relerr(zz.grad.cpu(), 3.0 * ref["grad"]) < 1e-5 and td.grad is None
        parts = crit.last_parts.cpu()
        assert crit.last_parts.is_cuda and abs(float(parts[0]) - float(ref["hard"])) < 2e-5 * max(1.0, abs(float(ref["hard"])))
        assert abs(float(parts[1]) - float(ref["kd"])) < 2e-5 * max(1.0, abs(float(ref["kd"])))
        hard = crit(z.cuda(), target)                         # a bare target: no teacher, the hard term alone
        assert abs(float(hard) - float(ref["hard"])) < 2e-5 * max(1.0, abs(float(ref["hard"]))) and float(crit.last_parts[1]) == 0.0
    crit.check_targets()
    bad = a.clone()
    bad[0] = Cn
    assert bool(torch.isnan(crit(z.cuda(), DistillTarget(bad.cuda(), t.cuda()))))
    with pytest.raises(ValueError):
        crit.check_targets()
    crit.check_targets()                                      # the flag was reset
    with pytest.raises(ValueError):
        crit(z.cuda(), DistillTarget(a.cuda(), t[:, :-1].contiguous().cuda()))   # a teacher with another class count
    with pytest.raises(RuntimeError):
        crit(z.cuda(), DistillTarget(a, t))                   # a target left on the host


# ---- determinism and meters --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cn", [(37, 257), (300, 5)])
def test_two_calls_give_identical_bytes_and_meters_match_the_soft_kernel(N, Cn):
    """two calls on the same inputs: identical bytes in every output, with and without meters, and the same bytes either way.  With
    meters: ranks and counts equal those of mnas_head_cross_entropy_soft on the same logits and labels; last_loss is the total"""
    from mnasnet_pytorch_amd.metrics import DeviceMeters
    z, t = BT.ce_logits("peak_on", N, Cn), BT.ce_logits("uniform4", N, Cn, seed=31)
    z[::2] = BT.ce_logits("uniform4", N, Cn)[::2]             # half the rows hit their label, the rest mostly miss
    a, b = BT.ce_targets(N, Cn)
    a = BT.ce_ignore(a, "third")
    lam, w = LAM[torch.arange(N) % 6].clone(), _weights(Cn, "zeros")
    dev, wt = _dev(z, a, b, lam), _dev(w, t)
    kd = BK.KD(N, Cn)
    runs = []
    mk, ms = DeviceMeters((1, 5)), DeviceMeters((1, 5))
    for meters in (None, None, mk, mk):
        res = kd.run(*dev, 0.1, *wt, 2.0, 0.5, meters=meters)
        res["ranks"] = kd.ranks.cpu().clone()
        runs.append(res)
    for r in runs[1:]:
        for k in ("dl", "rows", "parts"):
            G.bits_equal(r[k], runs[0][k], k)
        G.bits_equal(r["loss"].reshape(1), runs[0]["loss"].reshape(1), "loss")
    assert torch.equal(runs[2]["ranks"], runs[3]["ranks"])
    # the soft kernel on the same logits and labels, twice as well
    rows, loss = torch.empty(N, device="cuda"), torch.empty((), device="cuda")
    bad, ranks = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda")
    ks, nk, _, blk = ms.kernel_args(N, dev[0].device)
    for _ in range(2):
        L.check(L.load().mnas_head_cross_entropy_soft(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), 0.1, N, Cn,
                                                      -100, rows.data_ptr(), loss.data_ptr(), 0, bad.data_ptr(), ks, nk, ranks.data_ptr(),
                                                      blk, L.cur_stream()))
    assert torch.equal(runs[3]["ranks"], ranks.cpu())
    rk, rs = mk.read(), ms.read()
    print(rk, rs)
    assert rk.correct == rs.correct and rk.last_correct == rs.last_correct and (rk.steps, rk.samples) == (rs.steps, rs.samples) == (2, 2 * N)
    assert 0 < rk.correct[1] <= rk.correct[5] < rk.samples
    assert rk.last_loss == float(runs[3]["loss"]) and rk.loss.val == float(runs[3]["loss"]) and rk.nonfinite_steps == 0
