#!/usr/bin/env python3
"""What the multi-label recipe costs per step (a measurement helper: not a test, not bench.py).

MNASNet-1.0, head '512', bs 256, 224 x 224 uint8 batches (normalised on load), Adam, 600 classes, synthetic data, and three loops
timed as INTERLEAVED 40-step windows of one process (a difference counts only against the scatter of the same
code in the same call):

  A  native MultiClassBCELoss step (mnas_mlabel_bce)
  B  native MultiLabelLoss() step, everything off (mnas_mlabel_loss; bit for bit the same numbers as A)
  C  native MultiLabelLoss(gamma_neg=4, gamma_pos=1, margin=0.05, label_smoothing=0.1, pos_weight=...) step behind DeviceMix
     (Mixup and CutMix, one draw per image) on the label matrix: the mixing launch, the draws on the host and their one copy are
     part of C

Window order per round: A B A C, so every B and C window has an A window on either side.  Reported: ms/step of every window, the A-A
spread (adjacent A windows), B - A and C - A as paired differences against the mean of the two neighbouring A windows.  No threshold
is fixed in advance.

    python tools/mlabel_loss_overhead.py [--steps 40] [--rounds 5] [--out profiles/mlabel_loss_step.json]

The parent process never opens the GPU: it runs one child (--child) under its own `timeout -k 10`."""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("mlabel_loss_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from mnasnet_pytorch_amd import DeviceMix, FineTuneModelPool, MultiClassBCELoss, MultiLabelLoss, load_model
    from mnasnet_pytorch_amd.train_step import Trainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    random.seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        base = load_model("mnasnet")
    model = FineTuneModelPool(base, "mnasnet", args.classes, "512").to(dev).train()
    model.normalize_on_device()
    tr = Trainer(model, lr=1e-3)
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S, Cn = args.batch, args.size, args.classes
    x = torch.randint(0, 256, (B, 3, S, S), device=dev, generator=g, dtype=torch.uint8)
    Y = (torch.rand(B, Cn, device=dev, generator=g) < 0.02).float()
    pos_weight = 0.5 + 4.0 * torch.rand(Cn, generator=torch.Generator().manual_seed(5))
    crits = {"A": MultiClassBCELoss(), "B": MultiLabelLoss(),
             "C": MultiLabelLoss(gamma_neg=4, gamma_pos=1, margin=0.05, label_smoothing=0.1, pos_weight=pos_weight).to(dev)}
    mix = DeviceMix(mixup_alpha=0.2, cutmix_alpha=1.0, per_sample=True)

    def window(kind):
        tr.criterion = crits[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            if kind == "C":
                xm, ml = mix(x, Y)
                tr.step(xm, ml)
            else:
                tr.step(x, Y)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for k in "ABC":                                   # every shape and kernel of the three loops warm
        window(k)
        assert tr.last_logits is not None             # the native path was taken
    order = ["A", "B", "A", "C"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    a = [ms[i] for i, k in enumerate(order) if k == "A"]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = {k: [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, kk in enumerate(order) if kk == k] for k in ("B", "C")}
    r3 = lambda v: round(v, 4)                        # noqa: E731
    res = {
        "what": "multi-label step: native MultiClassBCELoss (A), native MultiLabelLoss() with everything off (B), native "
                "MultiLabelLoss(gamma_neg=4, gamma_pos=1, margin=0.05, label_smoothing=0.1, pos_weight) behind DeviceMix on the label "
                "matrix (C; the mixing launch and its host draws included)",
        "config": "MNASNet-1.0 + head '512', bs %d, %dx%d uint8, Adam, %d classes, synthetic data; %d steps per window, %d rounds of "
                  "A B A C, one process" % (B, S, S, Cn, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {k: [r3(ms[i]) for i, kk in enumerate(order) if kk == k] for k in ("A", "B", "C")},
        "ms_per_step_median": {k: r3(statistics.median(ms[i] for i, kk in enumerate(order) if kk == k)) for k in ("A", "B", "C")},
        "a_a_spread_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                          "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(statistics.median(paired["B"])), "paired": [r3(v) for v in paired["B"]]},
        "c_minus_a_ms": {"paired_median": r3(statistics.median(paired["C"])), "paired": [r3(v) for v in paired["C"]]},
    }
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=5, help="rounds of A B A C")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--classes", type=int, default=600)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds for the measuring process")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlabel_loss_step.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", "--classes", str(args.classes),
           "--steps", str(args.steps), "--rounds", str(args.rounds), "--batch", str(args.batch), "--size", str(args.size)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stdout.write(p.stdout[-4000:])
        sys.exit("the measuring process ended with status %d" % p.returncode)
    res = json.loads(line[-1][len("RESULT "):])
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
