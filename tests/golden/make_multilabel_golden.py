"""Writes tests/golden/multilabel.json: what the reference's own MultiClassBCELoss / HardDice (src/models/multi_class_loss.py),
batch_metrics (src/utils/metric.py; needs scikit-learn) and AverageMeter (src/train.py) give on the input grid of
tests/multilabel_ref.py.  Run where the reference checkout exists:

    python tests/golden/make_multilabel_golden.py <reference>/src

The two modules are loaded by path and AverageMeter is selected from train.py's syntax tree (train.py parses the command line at
import), at generation time only: the fixture holds RESULTS, nothing of the reference's text.  Per batch: the four loss variants
(plain, weighted, focal, weighted + focal) on fp32 inputs and again on the same inputs as fp64; HardDice(0.5) for both
deduct_intersection settings; the per-row F1 list of batch_metrics(target, sigmoid(out), threshold=0.5, f1_only=True) and
sum(list) / len(list) as train.py:457-463 forms it.  And one AverageMeter trace per meter of that branch.

train.py:456 reads `out = m(out)` with `m` undefined (the script would raise NameError there).  The fixture takes `m` to be the
torch.nn.Sigmoid() that the commented-out lines train.py:403 and :541 name (`# m = torch.nn.Sigmoid()`).

The script refuses to write unless, on every batch: the restatement's F1 rows and batch means equal the reference's EXACTLY, its Dice
is within 4 * 2^-24, no logit has 0 < |z| < 2^-20 (the device rules are on the logit and differ from an fp32 sigmoid below 2^-23), and
every fp64 BCE mean is >= 0.05 (so that the focal transform's 1 - pt does not cancel)."""
import ast
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import multilabel_ref as R  # noqa: E402


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_average_meter(train_py):
    tree = ast.parse(open(train_py).read(), train_py)
    picked = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "AverageMeter"]
    assert len(picked) == 1
    ns = {}
    exec(compile(ast.Module(body=picked, type_ignores=[]), train_py, "exec"), ns)
    return ns["AverageMeter"]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = sys.argv[1]
    torch.set_num_threads(1)
    warnings.simplefilter("ignore")
    ML = load_by_path("ref_multi_class_loss", os.path.join(src, "models", "multi_class_loss.py"))
    MT = load_by_path("ref_metric", os.path.join(src, "utils", "metric.py"))
    AverageMeter = reference_average_meter(os.path.join(src, "train.py"))
    m = torch.nn.Sigmoid()                                    # see the docstring
    crits = {name: ML.MultiClassBCELoss(use_weight_mask=wm, use_focal_weights=fo) for name, wm, fo in R.LOSS_VARIANTS}
    dices = {False: ML.HardDice(threshold=0.5, deduct_intersection=False), True: ML.HardDice(threshold=0.5, deduct_intersection=True)}
    batches = {}
    worst_f1 = worst_dice = 0.0
    min_z, min_b = float("inf"), float("inf")
    for C, scale, density, seed in R.grid():
        key = R.grid_key(C, scale, density, seed)
        z, t, w = R.grid_batch(C, scale, density, seed)
        az = z.abs()
        min_z = min(min_z, float(az[az > 0].min()))
        assert not bool(((az > 0) & (az < 2.0 ** -20)).any()), "a logit of %s is within 2^-20 of zero" % key
        rec = {"loss32": {}, "loss64": {}}
        for name, crit in crits.items():
            rec["loss32"][name] = float(crit(z, t, w))
            rec["loss64"][name] = float(crit(z.double(), t.double(), w.double()))
        for name in ("plain", "weighted"):
            min_b = min(min_b, rec["loss64"][name])
            assert rec["loss64"][name] >= 0.05, "BCE mean of %s (%s) is %g" % (key, name, rec["loss64"][name])
        rec["hdice"] = {str(d): float(dices[d](z, t)) for d in (False, True)}
        per_row = MT.batch_metrics(t, m(z), threshold=0.5, f1_only=True)              # one [f1] per sample (train.py:457-460)
        f1_of_rows = [row[0] for row in per_row]
        rec["f1_rows"] = [float(v) for v in f1_of_rows]
        rec["f1"] = float(sum(f1_of_rows) / len(f1_of_rows))                          # the batch value of train.py:463
        # ---- the check that fixed the grid
        ours_rows, ours_mean = R.f1_rows(z.numpy(), t.numpy()), R.f1_batch(z.numpy(), t.numpy())
        worst_f1 = max(worst_f1, max(abs(a - b) for a, b in zip(ours_rows, rec["f1_rows"])), abs(ours_mean - rec["f1"]))
        assert ours_rows == rec["f1_rows"] and ours_mean == rec["f1"], "F1 restatement vs reference on %s" % key
        for d in (False, True):
            diff = abs(R.hard_dice(z.numpy(), t.numpy(), 0.0, d) - rec["hdice"][str(d)])
            worst_dice = max(worst_dice, diff)
            assert diff <= 4 * 2.0 ** -24, "Dice restatement vs reference on %s: %g" % (key, diff)
        batches[key] = rec
    losses, dvals, f1s, ns, nf = R.meter_inputs()
    trace = {}
    for name, vals, nn in (("loss", losses, ns), ("hdice", dvals, ns), ("f1", f1s, nf)):
        am = AverageMeter()
        trace[name] = []
        for v, n in zip(vals, nn):
            am.update(v, n)
            trace[name].append({"val": am.val, "avg": am.avg, "sum": am.sum, "count": am.count})
    out = {"grid": {"C": list(R.GRID_C), "scale": list(R.GRID_SCALE), "density": list(R.GRID_DENSITY), "seeds": list(R.GRID_SEEDS),
                    "N": R.GRID_N},
           "batches": batches,
           "meter": {"loss": losses, "hdice": dvals, "f1": f1s, "n": ns, "n_f1": nf, "trace": trace}}
    with open(os.path.join(HERE, "multilabel.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote multilabel.json: %d batches; F1 difference %g, Dice difference <= %.3g, smallest |z| %.3g, smallest BCE mean %.4f"
          % (len(batches), worst_f1, worst_dice, min_z, min_b))


if __name__ == "__main__":
    main()
