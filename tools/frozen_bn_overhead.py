#!/usr/bin/env python3
"""What a training step on frozen BatchNorm statistics costs against the train-mode step (a measurement helper in the manner of
tools/meters_overhead.py: not a test, not bench.py, no gate).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224, Adam, synthetic inputs as bench.py builds them --
ONE model and trainer, two loops timed as INTERLEAVED windows in one process (a difference counts only against
the scatter of the same code in the same call):

  A  trainer.step, train mode                      (batch statistics: 57 finalize launches, statistics partials in every conv epilogue)
  B  trainer.step after model.freeze_bn()          (running statistics: one table launch, no partials, conv.bias gradients)

Window order A B A B ... A, so every B window has an A window on either side.  Reported: ms/step of every window, both medians, the
scatter of ADJACENT A windows (what "no difference" looks like here), B - A as paired differences against the mean of the two
neighbouring A windows, and `b_excess_over_a_scatter_ms` (how far the median paired difference lies above the largest adjacent A-A
difference; 0 when it does not).  Expected B <= A: the conv launches are the same.

    python tools/frozen_bn_overhead.py [--steps 40] [--rounds 8] [--out profiles/frozen_bn_step.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=8, help="rounds of A B")
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frozen_bn_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from meters_overhead import build
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, tr = build(dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)

    def window(kind):
        model.freeze_bn(kind == "B")
        assert tr._native_head() is not None and tr.engine.root.training == (kind == "A")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step(x, target)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for kind in ("A", "B"):                           # both programs built, every kernel warm
        for _ in range(max(1, args.warmup // args.steps)):
            window(kind)
    order = ["A", "B"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    model.freeze_bn(False)
    a = [v for v, k in zip(ms, order) if k == "A"]
    b = [v for v, k in zip(ms, order) if k == "B"]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, k in enumerate(order) if k == "B"]
    b_minus_a = statistics.median(paired)
    kinds = {}
    for key, lst in tr.engine.programs.items():
        kinds["frozen" if key[7] else "train"] = sum(p.fwd_n + p.bwd_all_n for p in lst)

    r3 = lambda v: round(v, 4)                        # noqa: E731
    res = {
        "what": "training step on frozen BatchNorm statistics (B) against the train-mode step (A), same model, interleaved windows",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d, Adam, synthetic data; %d steps per window, %d rounds of A B"
                  % (B, S, S, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {"A": [r3(v) for v in a], "B": [r3(v) for v in b]},
        "ms_per_step_median": {"A": r3(statistics.median(a)), "B": r3(statistics.median(b))},
        "a_a_scatter_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                           "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(b_minus_a), "paired": [r3(v) for v in paired]},
        "b_excess_over_a_scatter_ms": r3(max(0.0, b_minus_a - max(a_adj))),
        "launch_list_ops": kinds,
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
