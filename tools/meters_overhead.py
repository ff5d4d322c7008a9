#!/usr/bin/env python3
"""What the device meters cost and what they save (a measurement helper: not a test, not bench.py).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224, Adam, synthetic inputs as bench.py builds them --
and three loops, timed as INTERLEAVED windows in one process (a difference counts only against the scatter of
the same code in the same call):

  A  trainer.step only, meters = None                                  (what the step did before the meters existed)
  B  trainer.step with DeviceMeters, one read() per window            (train.py's print_freq read-back)
  C  trainer.step, then the reference's three lines per step: ATen softmax + top-k accuracy and three .item() host reads
     (train.py:447, 465-468)

Window order per round: A B A C, so every B and C window has an A window on either side.  Reported: ms/step of every window, the
A-A spread (adjacent A windows: what "no difference" looks like here), B - A and C - A as paired differences against the mean of the
two neighbouring A windows, and the verdict `b_within_a_spread` (|median paired B - A| <= the largest adjacent A-A difference).
Also: Trainer.validate images/s at the same batch (forward only), and the box's copy-bandwidth probe before and after.

    python tools/meters_overhead.py [--steps 40] [--rounds 8] [--out profiles/meters_overhead.json]

--trace-steps K [--with-meters]: no timing; K native steps at a small size after 3 warm-up steps, for a
`rocprofv3 --kernel-trace --stats` run that counts the launches of a step with and without meters."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(dev, classes=1000):
    from mnasnet_pytorch_amd import FineTuneModelPool, load_model
    from mnasnet_pytorch_amd.train_step import Trainer
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        base = load_model("mnasnet")
    model = FineTuneModelPool(base, "mnasnet", classes, "512").to(dev).train()
    return model, Trainer(model, lr=1e-3)


class HostMeter:
    """the running average train.py keeps on the host"""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def reference_lines(loss, logits, target, meters):
    """what train.py does after every step: three host reads and ATen softmax / topk / eq / sum in between"""
    n = target.size(0)
    meters[0].update(loss.item(), n)
    prob = torch.softmax(logits, 1)
    pred = prob.topk(5, 1, True, True)[1]
    hit = pred.eq(target.view(-1, 1))
    prec1 = hit[:, :1].float().sum() * (100.0 / n)
    prec5 = hit.float().sum() * (100.0 / n)
    meters[1].update(prec1.item(), n)
    meters[2].update(prec5.item(), n)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=8, help="rounds of A B A C")
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--val-batches", type=int, default=20)
    ap.add_argument("--no-box", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meters_overhead.json"))
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--with-meters", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("meters_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from mnasnet_pytorch_amd import DeviceMeters, _lib as L
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    if args.trace_steps:
        model, tr = build(dev, classes=10)
        tr.meters = DeviceMeters((1, 5), dev) if args.with_meters else None
        g = torch.Generator(device=dev).manual_seed(1234)
        x = torch.randn(32, 3, 64, 64, device=dev, generator=g)
        t = torch.randint(0, 10, (32,), device=dev, generator=g)
        for _ in range(3 + args.trace_steps):
            tr.step(x, t)
        torch.cuda.synchronize()
        print("traced %d steps after 3 warm-up steps, meters %s" % (args.trace_steps, "on" if args.with_meters else "off"))
        return

    box = None
    probe = None
    if not args.no_box:
        from bench import BoxProbe
        probe = BoxProbe(L.load(), dev)
        box = {"before": probe.measure()}
    model, tr = build(dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)
    meters = DeviceMeters((1, 5), dev)
    host = [HostMeter(), HostMeter(), HostMeter()]

    def window(kind):
        tr.meters = meters if kind == "B" else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = tr.step(x, target)
            if kind == "C":
                reference_lines(loss, tr.last_logits, target, host)
        if kind == "B":
            meters.read()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for kind in ("A", "B", "C"):                      # every shape and kernel of the three loops warm
        for _ in range(max(1, args.warmup // args.steps)):
            window(kind)
    for _ in range(args.warmup):
        tr.step(x, target)
    order = ["A", "B", "A", "C"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    tr.meters = None
    a_idx = [i for i, k in enumerate(order) if k == "A"]
    a = [ms[i] for i in a_idx]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = {k: [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, kk in enumerate(order) if kk == k] for k in ("B", "C")}
    med = {k: statistics.median(ms[i] for i, kk in enumerate(order) if kk == k) for k in ("A", "B", "C")}
    spread = max(a_adj)
    b_minus_a = statistics.median(paired["B"])

    # ---- validate: forward only
    val = [(x, target)] * args.val_batches
    tr.validate(val[:2])
    vw = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = tr.validate(val)                        # ends in read(): the one host sync
        vw.append(time.perf_counter() - t0)
    val_ips = B * args.val_batches / statistics.median(vw)
    if probe is not None:
        box["after"] = probe.measure()

    r3 = lambda v: round(v, 4)                        # noqa: E731
    res = {
        "what": "device meters: step time with (B) and without (A) them, and with the reference's three host reads per step (C)",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d, Adam, synthetic data; %d steps per window, %d rounds of A B A C"
                  % (B, S, S, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {k: [r3(ms[i]) for i, kk in enumerate(order) if kk == k] for k in ("A", "B", "C")},
        "ms_per_step_median": {k: r3(v) for k, v in med.items()},
        "a_a_spread_ms": {"adjacent_max": r3(spread), "adjacent_median": r3(statistics.median(a_adj)),
                          "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(b_minus_a), "paired": [r3(v) for v in paired["B"]]},
        "c_minus_a_ms": {"paired_median": r3(statistics.median(paired["C"])), "paired": [r3(v) for v in paired["C"]]},
        "b_within_a_spread": abs(b_minus_a) <= spread,
        "validate": {"images_per_s": round(val_ips, 1), "batches": args.val_batches, "batch": B, "size": S,
                     "window_s": [round(v, 4) for v in vw], "samples": rec.samples, "host_syncs_per_pass": 1},
        "meters_last_read": repr(meters.read()),
        "box": box,
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
