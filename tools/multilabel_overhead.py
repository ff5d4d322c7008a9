#!/usr/bin/env python3
"""What the multi-label branch costs on the device and what it saves (a measurement helper: not a test, not bench.py).

BASELINE configuration -- MNASNet-1.0, head '512', bs 256, 224 x 224, Adam, synthetic inputs as bench.py builds them -- at 90 and at
1000 classes, and three loops, timed as INTERLEAVED windows in one process per class count (a difference counts
only against the scatter of the same code in the same call):

  A  native cross-entropy step, meters = None
  B  native BCE step (MultiClassBCELoss) with MultiLabelMeters, one read() per window
  C  what the branch cost before: the same trainer with nn.BCEWithLogitsLoss through the module path (ATen + autograd for the head and
     the loss), then per step the N x C logits copied to the host and the per-row macro-F1 restated in numpy (the reference calls
     scikit-learn once per row there; scikit-learn is not needed here).  Nothing else: the reference's loss.item() and its HardDice
     with another .item() are left out, so C - A is the module path plus the F1 on the host, and B carries two meters more than C

Window order per round: A B A C, so every B and C window has an A window on either side.  Reported per class count: ms/step of every
window, the A-A spread (adjacent A windows), B - A and C - A as paired differences against the mean of the two neighbouring A windows,
and `b_within_a_spread` (|median paired B - A| <= the largest adjacent A-A difference).  No threshold is fixed in advance.

    python tools/multilabel_overhead.py [--steps 30] [--rounds 6] [--out profiles/multilabel_overhead.json]

The parent process never opens the GPU: it runs one child per class count (--child), each under its own `timeout -k 10`, and stops at
the first child that fails."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def f1_rows_host(pred, gt):
    """per row: macro-F1 over the labels present (pred, gt: bool [N][C]) -- what batch_metrics(f1_only=True) returns per sample"""
    out = []
    for p, y in zip(pred, gt):
        tp, fp, fn = int((p & y).sum()), int((p & ~y).sum()), int((~p & y).sum())
        tn = p.size - tp - fp - fn
        fs = []
        if tp + fp + fn > 0:
            fs.append(2 * tp / (2 * tp + fp + fn))
        if tn + fp + fn > 0:
            fs.append(2 * tn / (2 * tn + fp + fn))
        out.append(sum(fs) / len(fs))
    return out


def child(args):
    import torch
    import torch.nn as nn
    if not torch.cuda.is_available():
        sys.exit("multilabel_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from mnasnet_pytorch_amd import FineTuneModelPool, MultiClassBCELoss, MultiLabelMeters, load_model
    from mnasnet_pytorch_amd.train_step import Trainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        base = load_model("mnasnet")
    model = FineTuneModelPool(base, "mnasnet", args.classes, "512").to(dev).train()
    tr = Trainer(model, lr=1e-3)
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S, Cn = args.batch, args.size, args.classes
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    t_ce = torch.randint(0, Cn, (B,), device=dev, generator=g)
    t_ml = (torch.rand(B, Cn, device=dev, generator=g) < 0.05).float()
    crits = {"A": nn.CrossEntropyLoss(), "B": MultiClassBCELoss(), "C": nn.BCEWithLogitsLoss()}
    meters = MultiLabelMeters(dev)
    host_f1 = []
    seen = []
    model.register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))

    gt_host = t_ml.cpu().numpy() == 1                 # the labels are the loader's: they were on the host to begin with

    def f1_on_host(out):
        rows = f1_rows_host(torch.sigmoid(out).cpu().numpy() >= 0.5, gt_host)
        host_f1[:] = [sum(rows) / len(rows)]

    def window(kind):
        tr.criterion = crits[kind]
        tr.meters = meters if kind == "B" else None
        target = t_ce if kind == "A" else t_ml
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            seen.clear()
            tr.step(x, target)
            if kind == "C":
                f1_on_host(seen[-1])
        if kind == "B":
            meters.read()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    window("A")                                       # every shape and kernel of the three loops warm
    window("B")
    assert tr.last_logits is not None and not seen    # A and B took the native path (the module's forward never ran)
    window("C")
    assert seen
    order = ["A", "B", "A", "C"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    a = [ms[i] for i, k in enumerate(order) if k == "A"]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = {k: [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, kk in enumerate(order) if kk == k] for k in ("B", "C")}
    med = {k: statistics.median(ms[i] for i, kk in enumerate(order) if kk == k) for k in ("A", "B", "C")}
    spread = max(a_adj)
    b_minus_a = statistics.median(paired["B"])
    r3 = lambda v: round(v, 4)                        # noqa: E731
    res = {
        "classes": Cn,
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {k: [r3(ms[i]) for i, kk in enumerate(order) if kk == k] for k in ("A", "B", "C")},
        "ms_per_step_median": {k: r3(v) for k, v in med.items()},
        "a_a_spread_ms": {"adjacent_max": r3(spread), "adjacent_median": r3(statistics.median(a_adj)),
                          "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(b_minus_a), "paired": [r3(v) for v in paired["B"]]},
        "c_minus_a_ms": {"paired_median": r3(statistics.median(paired["C"])), "paired": [r3(v) for v in paired["C"]]},
        "b_within_a_spread": abs(b_minus_a) <= spread,
        "meters_last_read": repr(meters.read()),
        "host_f1_last": host_f1[0],
    }
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=30, help="steps per window")
    ap.add_argument("--rounds", type=int, default=6, help="rounds of A B A C")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--classes", type=int, default=0, help="(with --child) the class count of this process")
    ap.add_argument("--class-counts", type=int, nargs="+", default=[90, 1000])
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds for one class count")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilabel_overhead.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for Cn in args.class_counts:
        cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", "--classes", str(Cn),
               "--steps", str(args.steps), "--rounds", str(args.rounds), "--batch", str(args.batch), "--size", str(args.size)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stdout.write(p.stdout[-4000:])
            sys.exit("the run at %d classes ended with status %d: nothing further is started" % (Cn, p.returncode))
        runs.append(json.loads(line[-1][len("RESULT "):]))
        print(json.dumps(runs[-1]), flush=True)
    res = {
        "what": "multi-label branch: native cross-entropy step (A), native BCE step with MultiLabelMeters (B), and the module path with "
                "nn.BCEWithLogitsLoss plus, per step, the logits copied to the host and a per-row F1 in numpy (C; no loss.item() and no "
                "HardDice there, so C - A is the module path and the host F1 alone)",
        "config": "MNASNet-1.0 + head '512', bs %d, %dx%d, Adam, synthetic data; %d steps per window, %d rounds of A B A C, one process "
                  "per class count" % (args.batch, args.size, args.size, args.steps, args.rounds),
        "runs": runs,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
