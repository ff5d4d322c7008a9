#!/usr/bin/env python3
"""What global-norm gradient clipping, the non-finite skip and the weight EMA cost per training step (a measurement helper in the
manner of tools/frozen_bn_overhead.py: not a test, not bench.py, no gate and no threshold fixed in advance).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224, Adam, synthetic inputs as bench.py builds them --
ONE model and trainer; the three settings are plain attributes of the optimizer, switched between INTERLEAVED windows in one process
(a difference counts only against the scatter of the same code in the same call):

  A  trainer.step, all three off                   (the plain optimizer launch)
  B  clip_grad_norm on                             (+ one norm launch; the update runs as mnas_adam_step_ex)
  C  clip_grad_norm + skip_nonfinite + ema_decay   (+ the EMA shadow read and written in the update launch)

Window order A B A C A B A C ... A, so every B and C window has an A window on either side.  Reported: ms/step of every window, the
medians, the scatter of ADJACENT A windows (what "no difference" looks like here), B - A and C - A as paired differences against the
mean of the two neighbouring A windows, and next to them the traffic ESTIMATE (not measured): the norm pass reads 4n bytes, the EMA
adds 8n, n = trainable elements, at an assumed 4-6 TB/s, plus one launch (2.8-3.8 us measured in a stream).

    python tools/clip_ema_overhead.py [--steps 40] [--rounds 6] [--out profiles/clip_ema_step.json]"""
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
    ap.add_argument("--rounds", type=int, default=6, help="rounds of A B A C")
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--clip", type=float, default=1.0)
    ap.add_argument("--ema-decay", type=float, default=0.9999)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_ema_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_ema_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from meters_overhead import build
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, tr = build(dev)
    opt = tr.optimizer
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)
    settings = {"A": (None, False, None), "B": (args.clip, False, None), "C": (args.clip, True, args.ema_decay)}

    def window(kind):
        opt.clip_grad_norm, opt.skip_nonfinite, opt.ema_decay = settings[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step(x, target)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for kind in "ABC":                                # every kernel warm, the table, the stats block and the shadow allocated
        for _ in range(max(1, args.warmup // args.steps)):
            window(kind)
    order = ["A", "B", "A", "C"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    opt.clip_grad_norm, opt.skip_nonfinite, opt.ema_decay = settings["A"]
    stats = tr.grad_stats()
    by = {k: [v for v, o in zip(ms, order) if o == k] for k in "ABC"}
    a = by["A"]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = {k: [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, o in enumerate(order) if o == k] for k in "BC"}
    n = sum(b - a_ for a_, b in opt._trainable_runs())

    r3 = lambda v: round(v, 4)                        # noqa: E731
    us = lambda nbytes, tbps: round(nbytes / (tbps * 1e12) * 1e6, 2)      # noqa: E731
    res = {
        "what": "training step with gradient clipping (B) and with clipping + non-finite skip + weight EMA (C) against the plain step "
                "(A), same model and trainer, interleaved windows",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d, Adam, synthetic data; clip_grad_norm %g, ema_decay %g; %d steps "
                  "per window, %d rounds of A B A C" % (B, S, S, args.clip, args.ema_decay, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {k: [r3(v) for v in by[k]] for k in "ABC"},
        "ms_per_step_median": {k: r3(statistics.median(by[k])) for k in "ABC"},
        "a_a_scatter_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                           "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(statistics.median(paired["B"])), "paired": [r3(v) for v in paired["B"]]},
        "c_minus_a_ms": {"paired_median": r3(statistics.median(paired["C"])), "paired": [r3(v) for v in paired["C"]]},
        "traffic_estimate_not_measured": {
            "trainable_elements": n,
            "norm_pass_read_bytes": 4 * n, "ema_extra_bytes": 8 * n,
            "norm_pass_us_at_4_to_6_TBps": [us(4 * n, 6), us(4 * n, 4)],
            "ema_extra_us_at_4_to_6_TBps": [us(8 * n, 6), us(8 * n, 4)],
            "launch_us_measured_in_a_stream": [2.8, 3.8],
        },
        "grad_stats": stats._asdict(),
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
