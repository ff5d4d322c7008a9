"""CPU (no GPU needed): the restatement of the meters (tests/metrics_ref.py) equals, exactly, what the reference's accuracy() and
AverageMeter recorded in tests/golden/metrics.json on every batch of the grid; the MnasMeters block has the header's layout; the
new entry points are declared, exported and typed; the Python surface exists and refuses to run without an MI355X."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "metrics.json")))


def test_fixture_covers_the_whole_grid():
    g = GOLD["grid"]
    assert (tuple(g["C"]), tuple(g["scale"]), tuple(g["seeds"]), g["N"]) == (R.GRID_C, R.GRID_SCALE, R.GRID_SEEDS, R.GRID_N)
    assert sorted(GOLD["batches"]) == sorted(R.grid_key(*c) for c in R.grid()) and len(GOLD["batches"]) == 90


@pytest.mark.parametrize("C", R.GRID_C)
@pytest.mark.parametrize("scale", R.GRID_SCALE)
def test_rank_rule_and_argsort_equal_reference(C, scale):
    """every batch, none left out: the rank rule on the LOGITS gives the reference's prec@1 / prec@5 on the logits and on the fp32
    softmax; so does the argsort + membership restatement of accuracy()"""
    for seed in R.GRID_SEEDS:
        z, t = R.grid_batch(C, scale, seed)
        ref = GOLD["batches"][R.grid_key(C, scale, seed)]
        c = R.correct_counts(z.numpy(), t.numpy(), (1, 5))
        ours = [c[1] * 100.0 / R.GRID_N, c[5] * 100.0 / R.GRID_N]
        assert ours == [ref["prec1"], ref["prec5"]] == [ref["prec1_softmax"], ref["prec5_softmax"]], (C, scale, seed)
        assert R.precision_at_k(z.numpy(), t.numpy(), (1, 5)) == [ref["prec1"], ref["prec5"]]
        assert R.precision_at_k(torch.softmax(z, 1).numpy(), t.numpy(), (1, 5)) == [ref["prec1_softmax"], ref["prec5_softmax"]]
        assert 0 < c[1] <= c[5] < R.GRID_N            # the grid is neither trivial nor saturated


def test_rank_rule_ties_and_bad_rows():
    z = torch.tensor([[1.0, 2.0, 2.0, 2.0, 0.0, 2.0, 2.0, 2.0]] * 4 + [[0.0, float("nan"), 1.0, 0, 0, 0, 0, 0]] * 2)
    t = torch.tensor([1, 3, 7, 0, 1, 8])
    assert R.ranks(z.numpy(), t.numpy()).tolist() == [0, 2, 5, 6, R.WRONG, R.WRONG]
    assert R.correct_counts(z.numpy(), t.numpy(), (1, 5, 100)) == {1: 1, 5: 2, 100: 4}
    assert R.correct_counts(z.numpy(), torch.tensor([1, -100, 7, 0, 1, 8]).numpy(), (5,), ignore_index=-100) == {5: 1}


def test_meter_arithmetic_equals_reference():
    vals, ns = R.meter_inputs(GOLD["meter"]["seed"], len(GOLD["meter"]["trace"]))
    assert vals == GOLD["meter"]["values"] and ns == GOLD["meter"]["n"]
    m = R.Meter()
    for v, n, want in zip(vals, ns, GOLD["meter"]["trace"]):
        m.update(v, n)
        assert m.state() == want


def test_meters_block_layout_and_symbols():
    from mnasnet_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mnas.h")).read()
    body = re.search(r"typedef struct MnasMeters \{(.*?)\} MnasMeters;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int64_t|double)\s+(\w+)(?:\[(\w+)\])?;", body)
    macro = {m: int(v) for m, v in re.findall(r"#define (MNAS_METERS_\w+)\s+(\d+)", hdr)}
    assert (macro["MNAS_METERS_MAX_K"], macro["MNAS_METERS_NUM_I64"], macro["MNAS_METERS_NUM_F64"]) == \
        (_lib.METERS_MAX_K, _lib.METERS_NUM_I64, _lib.METERS_NUM_F64)
    flat = [(ty, name, macro[dim] if dim in macro else int(dim or 1)) for ty, name, dim in fields]
    assert [(n, c) for _, n, c in flat] == [(n, getattr(t, "_length_", 1)) for n, t in _lib.MnasMeters._fields_]
    for (ty, _, _), (_, ct) in zip(flat, _lib.MnasMeters._fields_):
        base = getattr(ct, "_type_", ct) if hasattr(ct, "_length_") else ct
        assert base is (ctypes.c_int64 if ty == "int64_t" else ctypes.c_double)
    n_i64 = sum(c for ty, _, c in flat if ty == "int64_t")
    n_f64 = sum(c for ty, _, c in flat if ty == "double")
    assert (n_i64, n_f64) == (_lib.METERS_NUM_I64, _lib.METERS_NUM_F64)
    assert [ty for ty, _, _ in flat] == sorted((ty for ty, _, _ in flat), key=lambda s: s != "int64_t")   # all int64 first
    assert ctypes.sizeof(_lib.MnasMeters) == 8 * (n_i64 + n_f64) == 136
    assert _lib.MnasMeters.loss_sum.offset == 8 * n_i64 and _lib.MnasMeters.last_correct.offset == 8 * (n_i64 - _lib.METERS_MAX_K)
    lib = _lib.load()
    for name in ("mnas_head_cross_entropy_metrics", "mnas_head_metrics"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert len(_lib.SYMBOLS["mnas_head_cross_entropy_metrics"][1]) == 14 and len(_lib.SYMBOLS["mnas_head_metrics"][1]) == 10
    assert lib.mnas_version() == _lib.ABI_VERSION == 8
    # argument checks run on the host before anything is launched
    ks = (ctypes.c_int * 2)(1, 5)
    assert lib.mnas_head_metrics(None, None, 4, 10, ks, 2, None, None, None, None) == _lib.EINVAL


def test_python_surface():
    import mnasnet_pytorch_amd as P
    from mnasnet_pytorch_amd.head import NativeHead
    from mnasnet_pytorch_amd.metrics import MetersRecord
    from mnasnet_pytorch_amd.train_step import Trainer
    assert "DeviceMeters" in P.__all__ and "accuracy" in P.__all__
    assert list(inspect.signature(P.DeviceMeters.__init__).parameters)[1:] == ["topk", "device"]
    assert inspect.signature(P.DeviceMeters.__init__).parameters["topk"].default == (1, 5)
    assert list(inspect.signature(P.accuracy).parameters) == ["output", "target", "topk"]
    assert list(inspect.signature(Trainer.validate).parameters)[1:] == ["batches", "meters", "transform", "max_batches", "reduce"]
    assert inspect.signature(Trainer.__init__).parameters["meters"].default is None
    for fn in (NativeHead.cross_entropy, NativeHead.loss_and_grad):
        assert inspect.signature(fn).parameters["meters"].default is None
    with pytest.raises(RuntimeError):
        P.DeviceMeters(device="cpu")                 # no CPU path
    with pytest.raises(ValueError):
        P.DeviceMeters(topk=(1, 2, 3, 4, 5), device="cuda:0")
    # decoding a block: AverageMeter / accuracy() arithmetic
    from mnasnet_pytorch_amd import _lib
    raw = _lib.MnasMeters()
    raw.steps, raw.samples, raw.loss_samples, raw.last_n, raw.last_loss_n = 2, 356, 356, 100, 100
    raw.correct[0], raw.correct[1], raw.last_correct[0], raw.last_correct[1] = 89, 178, 10, 50
    raw.loss_sum, raw.last_loss, raw.last_loss_sum = 2.5 * 256 + 0.75 * 100, 0.75, 75.0
    rec = MetersRecord(raw, (1, 5))
    assert (rec.loss.val, rec.loss.avg) == (0.75, (2.5 * 256 + 0.75 * 100) / 356)
    assert (rec.acc[1].val, rec.acc[1].avg, rec.acc[5].val, rec.acc[5].avg) == (10.0, 25.0, 50.0, 50.0)
