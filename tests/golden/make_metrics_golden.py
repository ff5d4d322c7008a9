"""Writes tests/golden/metrics.json: what the reference's own accuracy() and AverageMeter (src/train.py:657-700) give on the input
grid of tests/metrics_ref.py.  Run where the reference checkout exists:

    python tests/golden/make_metrics_golden.py <reference>/src/train.py

train.py cannot be imported (it parses the command line and pulls in TensorBoard at import), so the two definitions are selected
from its syntax tree and compiled on their own, at generation time only: the fixture holds seeds and RESULTS, nothing of the
reference's text.  For every batch of the grid: prec@1 / prec@5 on the logits and on torch.softmax(logits, 1) (what train.py:589-590
feeds it); and an AverageMeter's val / avg / sum / count after each of ten updates.  The script also repeats the check that
fixed the grid: on every batch the rank rule on the logits must give the reference's counts, on logits and softmax alike, with
no batch left out -- it refuses to write the fixture otherwise.

accuracy() is 2018 code: `correct[:k].view(-1)` views rows of a transposed tensor, which current PyTorch refuses ("view size is not
compatible with input tensor's size and stride").  The syntax tree's `.view(` calls inside accuracy() are therefore renamed to
`.reshape(` before compiling -- the same elements in the same order, the fix PyTorch's own message asks for."""
import ast
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_ref as R  # noqa: E402


def reference_definitions(train_py):
    tree = ast.parse(open(train_py).read(), train_py)
    want = {"accuracy": ast.FunctionDef, "AverageMeter": ast.ClassDef}
    picked = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and isinstance(n, want.get(n.name, ()))]
    assert sorted(n.name for n in picked) == sorted(want), [n.name for n in picked]
    for n in picked:
        if n.name == "accuracy":
            for a in ast.walk(n):
                if isinstance(a, ast.Attribute) and a.attr == "view":
                    a.attr = "reshape"
    ns = {"torch": torch}
    exec(compile(ast.Module(body=picked, type_ignores=[]), train_py, "exec"), ns)
    return ns["accuracy"], ns["AverageMeter"]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    torch.set_num_threads(1)
    accuracy, AverageMeter = reference_definitions(sys.argv[1])
    batches = {}
    for C, scale, seed in R.grid():
        z, t = R.grid_batch(C, scale, seed)
        p1, p5 = (float(v) for v in accuracy(z, t, topk=(1, 5)))
        s1, s5 = (float(v) for v in accuracy(torch.softmax(z, 1), t, topk=(1, 5)))
        ours = R.correct_counts(z.numpy(), t.numpy(), (1, 5))
        for name, got in (("logits", (p1, p5)), ("softmax", (s1, s5))):
            want = tuple(ours[k] * 100.0 / R.GRID_N for k in (1, 5))
            assert got == want, "rank rule vs reference on %s of %s: %r != %r" % (name, R.grid_key(C, scale, seed), want, got)
        batches[R.grid_key(C, scale, seed)] = {"prec1": p1, "prec5": p5, "prec1_softmax": s1, "prec5_softmax": s5}
    vals, ns = R.meter_inputs()
    m = AverageMeter()
    trace = []
    for v, n in zip(vals, ns):
        m.update(v, n)
        trace.append({"val": m.val, "avg": m.avg, "sum": m.sum, "count": m.count})
    out = {"grid": {"C": list(R.GRID_C), "scale": list(R.GRID_SCALE), "seeds": list(R.GRID_SEEDS), "N": R.GRID_N},
           "batches": batches, "meter": {"seed": 1234, "values": vals, "n": ns, "trace": trace}}
    with open(os.path.join(HERE, "metrics.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote metrics.json: %d batches, %d meter updates" % (len(batches), len(trace)))


if __name__ == "__main__":
    main()
