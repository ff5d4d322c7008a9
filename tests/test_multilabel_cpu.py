"""CPU (no GPU needed): the restatement of the multi-label branch (tests/multilabel_ref.py) equals what the reference's
MultiClassBCELoss / HardDice / batch_metrics / AverageMeter recorded in tests/golden/multilabel.json on every batch of the grid (F1
exactly, Dice within 4 * 2^-24, the fp64 losses within 1e-12); hand-made edge rows; the MnasMultiLabelMeters block has the header's
layout; the new entry points are declared, exported, typed and check their arguments on the host; the Python surface exists and
refuses to run without an MI355X."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import multilabel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "multilabel.json")))
DICE_TOL = 4 * 2.0 ** -24


def test_fixture_covers_the_whole_grid():
    g = GOLD["grid"]
    assert (tuple(g["C"]), tuple(g["scale"]), tuple(g["density"]), tuple(g["seeds"]), g["N"]) == \
        (R.GRID_C, R.GRID_SCALE, R.GRID_DENSITY, R.GRID_SEEDS, R.GRID_N)
    assert sorted(GOLD["batches"]) == sorted(R.grid_key(*c) for c in R.grid()) and len(GOLD["batches"]) == 90


@pytest.mark.parametrize("C", R.GRID_C)
@pytest.mark.parametrize("scale", R.GRID_SCALE)
def test_restatement_equals_reference(C, scale):
    for density in R.GRID_DENSITY:
        for seed in R.GRID_SEEDS:
            key = R.grid_key(C, scale, density, seed)
            ref = GOLD["batches"][key]
            z, t, w = (a.numpy() for a in R.grid_batch(C, scale, density, seed))
            az = np.abs(z)
            assert not ((az > 0) & (az < 2.0 ** -20)).any(), key          # the rules on the logit equal the rules on the sigmoid
            assert R.f1_rows(z, t) == ref["f1_rows"], key
            assert R.f1_batch(z, t) == ref["f1"], key
            for d in (False, True):
                assert abs(R.hard_dice(z, t, 0.0, d) - ref["hdice"][str(d)]) <= DICE_TOL, (key, d)
            for name, weighted, focal in R.LOSS_VARIANTS:
                ours = R.bce(z, t, w if weighted else None, focal)[0]
                want = ref["loss64"][name]
                assert abs(ours - want) <= 1e-12 * abs(want), (key, name, ours, want)
                assert abs(ref["loss32"][name] - want) <= 2e-5 * abs(want), (key, name)    # the fp32 reference itself
            assert ref["loss64"]["plain"] >= 0.05 and ref["loss64"]["weighted"] >= 0.05


def test_gradient_of_the_restatement():
    """the closed-form gradient of all four variants equals autograd's on the same formula in float64"""
    z, t, w = R.grid_batch(90, 2.0, 0.3, 0)
    for name, weighted, focal in R.LOSS_VARIANTS:
        zr = z.double().requires_grad_(True)
        b = torch.nn.functional.binary_cross_entropy_with_logits(zr, t.double(), weight=w.double() if weighted else None)
        loss = R.BALANCE * (1 - torch.exp(-b)) ** R.FOCUS * b if focal else b
        loss.backward()
        ours, g = R.bce(z.numpy(), t.numpy(), w.numpy() if weighted else None, focal)
        assert abs(ours - float(loss.detach())) <= 1e-12 * abs(float(loss.detach())), name
        assert np.abs(g - zr.grad.numpy()).max() <= 1e-12 * np.abs(g).max(), name


def test_edge_rows():
    one = lambda z, t: (R.f1_rows(np.array([z], np.float32), np.array([t], np.float32))[0],       # noqa: E731
                        R.hard_dice(np.array([z], np.float32), np.array([t], np.float32)))
    # z == 0 with t == 1: F1 counts it as predicted (tp = 1, nothing else -> 1.0), Dice does not (I = 0 -> 0)
    assert one([0.0], [1.0]) == (1.0, 0.0)
    assert R.dice_counts(np.array([[0.0]], np.float32), np.array([[1.0]], np.float32)) == (0, 0, 1)
    # all-negative logits and all-zero targets: only label 0 occurs, perfectly -> 1; nothing hit -> Dice 0
    assert one([-1.0, -2.0, -0.5], [0.0, 0.0, 0.0]) == (1.0, 0.0)
    # everything right
    assert one([3.0, -3.0, 2.0, -1.0], [1.0, 0.0, 1.0, 0.0]) == (1.0, 1.0)
    # everything wrong
    assert one([-3.0, 3.0, -2.0, 1.0], [1.0, 0.0, 1.0, 0.0]) == (0.0, 0.0)
    # a NaN logit is predicted negative under both rules; a soft target is a negative for the metrics
    assert R.dice_counts(np.array([[np.nan, 1.0, 1.0]], np.float32), np.array([[1.0, 0.3, 1.0]], np.float32)) == (1, 1, 1)
    f, d = one([np.nan, 1.0, 1.0], [1.0, 0.3, 1.0])
    assert f == (2 * 1 / (2 * 1 + 1 + 1) + 0.0) / 2 and abs(d - (1 + np.log(2 / 4))) <= DICE_TOL
    # deduct_intersection: U = 2 + 2 - 1
    assert abs(R.hard_dice(np.array([[np.nan, 1.0, 1.0]], np.float32), np.array([[1.0, 0.3, 1.0]], np.float32), 0.0, True)
               - (1 + np.log(2 / 3))) <= DICE_TOL


def test_meter_arithmetic_equals_reference():
    losses, dices, f1s, ns, nf = R.meter_inputs(len(GOLD["meter"]["n"]))
    g = GOLD["meter"]
    assert (losses, dices, f1s, ns, nf) == (g["loss"], g["hdice"], g["f1"], g["n"], g["n_f1"])
    for name, vals, nn in (("loss", losses, ns), ("hdice", dices, ns), ("f1", f1s, nf)):
        m = R.Meter()
        for v, n, want in zip(vals, nn, g["trace"][name]):
            m.update(v, n)
            assert m.state() == want, name


def test_block_layout_and_symbols():
    from mnasnet_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mnas.h")).read()
    body = re.search(r"typedef struct MnasMultiLabelMeters \{(.*?)\} MnasMultiLabelMeters;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int64_t|double)\s+(\w+);", body)
    macro = {m: int(v) for m, v in re.findall(r"#define (MNAS_MLABEL_\w+)\s+(\d+)", hdr)}
    assert (macro["MNAS_MLABEL_NUM_I64"], macro["MNAS_MLABEL_NUM_F64"]) == (_lib.MLABEL_NUM_I64, _lib.MLABEL_NUM_F64) == (16, 9)
    assert [n for _, n in fields] == [n for n, _ in _lib.MnasMultiLabelMeters._fields_]
    for (ty, _), (_, ct) in zip(fields, _lib.MnasMultiLabelMeters._fields_):
        assert ct is (ctypes.c_int64 if ty == "int64_t" else ctypes.c_double)
    tys = [ty for ty, _ in fields]
    assert tys == ["int64_t"] * 16 + ["double"] * 9                                 # all int64 first: an all-reduce is two tensors
    assert ctypes.sizeof(_lib.MnasMultiLabelMeters) == 8 * 25 == 200
    assert _lib.MnasMultiLabelMeters.loss_sum.offset == 8 * 16
    for want in ("steps", "samples", "nonfinite_steps", "tp", "fp", "fn", "loss_sum", "dice_sum", "f1_sum", "last_loss", "last_dice",
                 "last_f1"):
        assert want in [n for _, n in fields]
    # the earlier block and the ABI version are untouched
    assert ctypes.sizeof(_lib.MnasMeters) == 136
    lib = _lib.load()
    assert lib.mnas_version() == _lib.ABI_VERSION == 8
    for name, nargs in (("mnas_mlabel_bce", 16), ("mnas_mlabel_metrics", 11), ("mnas_mlabel_hard_dice", 9), ("mnas_mlabel_scratch_bytes", 1)):
        assert re.search(r"\b(int|int64_t) %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(_lib.SYMBOLS[name][1]) == nargs
    src = open(os.path.join(ROOT, "mnasnet_pytorch_amd", "csrc", "Makefile")).read()
    assert "mnas_mlabel.hip" in src


def test_host_argument_checks():
    """every entry point refuses bad arguments on the host, before any launch (no GPU is touched: all return EINVAL first)"""
    from mnasnet_pytorch_amd import _lib
    lib = _lib.load()
    E = _lib.EINVAL
    p = 4096                                           # a non-NULL, 16-byte aligned "pointer": never dereferenced on these paths
    assert lib.mnas_mlabel_scratch_bytes(12) >= 24 * 12 and lib.mnas_mlabel_scratch_bytes(0) == 0
    assert lib.mnas_mlabel_bce(None, p, None, 4, 10, 0, 2.0, 0.25, p, p, None, None, 0, 0, 0, None) == E       # logits
    assert lib.mnas_mlabel_bce(p, None, None, 4, 10, 0, 2.0, 0.25, p, p, None, None, 0, 0, 0, None) == E       # target
    assert lib.mnas_mlabel_bce(p, p, None, 4, 10, 0, 2.0, 0.25, None, p, None, None, 0, 0, 0, None) == E       # scratch
    assert lib.mnas_mlabel_bce(p, p, None, 4, 10, 0, 2.0, 0.25, p, None, None, None, 0, 0, 0, None) == E       # loss
    assert lib.mnas_mlabel_bce(p, p, None, 0, 10, 0, 2.0, 0.25, p, p, None, None, 0, 0, 0, None) == E          # N
    assert lib.mnas_mlabel_bce(p, p, None, 4, 0, 0, 2.0, 0.25, p, p, None, None, 0, 0, 0, None) == E           # C
    assert lib.mnas_mlabel_bce(p, p, None, 4, 10, 1, 0.5, 0.25, p, p, None, None, 0, 0, 0, None) == E          # focal, gamma < 1
    assert lib.mnas_mlabel_bce(p, p, None, 4, 10, 1, float("nan"), 0.25, p, p, None, None, 0, 0, 0, None) == E
    assert lib.mnas_mlabel_bce(p, p, None, 4, 10, 0, 2.0, 0.25, p + 4, p, None, None, 0, 0, 0, None) == E      # scratch alignment
    assert lib.mnas_mlabel_bce(p, p, None, 4, 10, 0, 2.0, 0.25, p, p, None, p, -1, 4, 4, None) == E            # meter weight < 0
    assert lib.mnas_mlabel_metrics(None, None, 4, 10, None, None, None, 4, 4, 4, None) == E
    assert lib.mnas_mlabel_metrics(p, p, 4, 10, None, p, None, 4, 4, 4, None) == E                             # no block
    assert lib.mnas_mlabel_metrics(p, p, 4, 10, None, p, p, 4, 4, -3, None) == E
    assert lib.mnas_mlabel_hard_dice(p, p, 4, 10, 0.0, 0, p, None, None) == E                                  # out
    assert lib.mnas_mlabel_hard_dice(p, p, 0, 10, 0.0, 0, p, p, None) == E
    assert lib.mnas_mlabel_hard_dice(p, p, 4, 10, float("nan"), 0, p, p, None) == E


def test_criterion_checks_and_routing():
    """the criterion's own checks come in one order whatever the input's rank, and only the class itself is routed natively"""
    import types
    import mnasnet_pytorch_amd as P
    from mnasnet_pytorch_amd.train_step import Trainer
    crit = P.MultiClassBCELoss(use_weight_mask=True)
    for shape in ((3,), (2, 3, 4)):
        with pytest.raises(ValueError):                     # outputs that are not (N, C), before any size(1)
            crit(torch.zeros(shape), torch.zeros(shape))
    for tshape in ((2,), (3, 3), (2, 4), (2, 3, 1)):
        with pytest.raises(AssertionError):                 # rank, rows, classes of the target
            crit(torch.zeros(2, 3), torch.zeros(tshape))
    for wshape in ((2,), (3, 3), (2, 4)):
        for c in (crit, P.MultiClassBCELoss()):             # checked whether or not the weights are used
            with pytest.raises(ValueError):
                c(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(wshape))

    class Mine(P.MultiClassBCELoss):
        def forward(self, outputs, targets, weights=None):
            return super().forward(outputs, targets, weights) * 2

    assert Trainer._multilabel(types.SimpleNamespace(criterion=P.MultiClassBCELoss()))
    assert not Trainer._multilabel(types.SimpleNamespace(criterion=Mine()))
    assert not Trainer._multilabel(types.SimpleNamespace(criterion=torch.nn.BCEWithLogitsLoss()))
    # a meters object of the wrong kind is refused for the class and for its subclasses alike (it could count nothing)
    for c in (P.MultiClassBCELoss(), Mine()):
        with pytest.raises(ValueError):
            Trainer._check_meters(types.SimpleNamespace(criterion=c), object())
        Trainer._check_meters(types.SimpleNamespace(criterion=c), None)


def test_python_surface():
    import mnasnet_pytorch_amd as P
    from mnasnet_pytorch_amd.head import NativeHead
    from mnasnet_pytorch_amd.metrics import MeterValue, MultiLabelRecord
    for name in ("MultiClassBCELoss", "HardDice", "MultiLabelMeters"):
        assert name in P.__all__ and hasattr(P, name)
    sig = inspect.signature(P.MultiClassBCELoss.__init__).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("use_weight_mask", False), ("use_focal_weights", False),
                                                                  ("focus_param", 2), ("balance_param", 0.25)]
    sig = inspect.signature(P.MultiClassBCELoss.forward).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("outputs", inspect.Parameter.empty), ("targets", inspect.Parameter.empty),
                                                                  ("weights", None)]
    sig = inspect.signature(P.HardDice.__init__).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("threshold", 0.5), ("deduct_intersection", False)]
    assert list(inspect.signature(P.HardDice.forward).parameters)[1:] == ["outputs", "targets"]
    assert list(inspect.signature(P.MultiLabelMeters.__init__).parameters)[1:] == ["device"]
    sig = inspect.signature(P.MultiLabelMeters.update).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("logits", inspect.Parameter.empty), ("target", inspect.Parameter.empty),
                                                                  ("loss", None), ("f1_n", None)]
    for m in ("read", "reset", "all_reduce", "kernel_args"):
        assert callable(getattr(P.MultiLabelMeters, m))
    assert callable(NativeHead.bce) and "criterion" in inspect.signature(NativeHead.loss_and_grad).parameters
    # no CPU path
    crit = P.MultiClassBCELoss()
    with pytest.raises(RuntimeError):
        crit(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(AssertionError):
        crit(torch.zeros(2, 3), torch.zeros(2, 4))           # the reference's shape asserts come first
    with pytest.raises(RuntimeError):
        P.HardDice()(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(RuntimeError):
        P.MultiLabelMeters(device="cpu")
    # documented deviations
    with pytest.raises(ValueError):
        P.MultiClassBCELoss(use_focal_weights=True, focus_param=0.5)
    for th in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            P.HardDice(threshold=th)
    P.MultiClassBCELoss(use_focal_weights=True, focus_param=1)
    P.HardDice(threshold=0.3, deduct_intersection=True)
    # decoding a block: AverageMeter arithmetic; val of one rank is the stored value, of a reduced block the weighted mean
    from mnasnet_pytorch_amd import _lib
    raw = _lib.MnasMultiLabelMeters()
    raw.steps, raw.samples, raw.tp, raw.fp, raw.fn = 2, 356, 7, 5, 3
    raw.loss_n, raw.dice_n, raw.f1_n, raw.last_loss_n, raw.last_dice_n, raw.last_f1_n = 356, 356, 6, 100, 100, 3
    raw.loss_sum, raw.last_loss, raw.last_loss_sum = 2.5 * 256 + 0.75 * 100, 0.75, 75.0
    raw.dice_sum, raw.last_dice, raw.last_dice_sum = 0.5 * 256 + 0.25 * 100, 0.25, 25.0
    raw.f1_sum, raw.last_f1, raw.last_f1_sum = 0.1 * 3 + 0.7 * 3, 0.7, 0.7 * 3
    rec = MultiLabelRecord(raw)
    assert isinstance(rec.loss, MeterValue) and (rec.loss.val, rec.loss.avg) == (0.75, (2.5 * 256 + 0.75 * 100) / 356)
    assert (rec.hdice.val, rec.hdice.avg) == (0.25, (0.5 * 256 + 0.25 * 100) / 356)
    assert (rec.f1.val, rec.f1.avg) == (0.7, (0.1 * 3 + 0.7 * 3) / 6)
    assert (rec.tp, rec.fp, rec.fn, rec.steps, rec.samples, rec.nonfinite_steps) == (7, 5, 3, 2, 356, 0)
    raw.last_f1, raw.last_f1_sum, raw.last_f1_n = 0.7 + 0.2, 0.7 * 3 + 0.2 * 5, 8           # two ranks' last updates, summed
    assert MultiLabelRecord(raw).f1.val == (0.7 * 3 + 0.2 * 5) / 8
