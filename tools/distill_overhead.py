#!/usr/bin/env python3
"""What knowledge distillation costs per training step (a measurement helper in the manner of tools/mix_overhead.py: not a test, not
bench.py, no gate and no threshold fixed in advance).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224, Adam -- on a uint8 batch (normalisation in the
stem's input load).  ONE student model and trainer and ONE teacher of the same architecture; criterion and teacher are plain
attributes of the trainer, switched between INTERLEAVED windows in one process (a difference counts only against
the scatter of the same code in the same call):

  A  trainer.step(x, target), nn.CrossEntropyLoss()                                            (the plain native step)
  B  teacher(x) in eval mode under no_grad, logits thrown away; then A                        (the plain step plus a teacher forward)
  C  trainer.step(x, target), DistillCrossEntropyLoss(T, alpha, eps, weight=w), teacher=...   (the distilled step)

C - B is the cost of the loss itself (two launches of mnas_head_cross_entropy_kd in place of two of mnas_head_cross_entropy, plus
the wrapping of the target); B - A is the teacher's forward.  Window order A B A C A B A C ... A, so every B and C window has an A
window on either side.  Reported: ms/step of every window, the medians, the scatter of ADJACENT A windows (what "no difference" looks
like here), B - A and C - A as paired differences against the mean of the two neighbouring A windows, and C - B from the paired
medians.

    python tools/distill_overhead.py [--steps 40] [--rounds 6] [--out profiles/distill_step.json]"""
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
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--smoothing", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distill_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from meters_overhead import build
    from mnasnet_pytorch_amd import DistillCrossEntropyLoss
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, tr = build(dev)
    model.normalize_on_device()
    teacher, _ = build(dev)                           # same architecture, its own weights and engine; never stepped
    teacher.normalize_on_device()
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)
    weight = torch.rand(1000, device=dev, generator=g) + 0.5
    plain = torch.nn.CrossEntropyLoss()
    distill = DistillCrossEntropyLoss(args.temperature, args.alpha, args.smoothing, weight=weight)

    def teacher_forward():
        teacher.eval()
        with torch.no_grad():
            teacher(x)
        teacher.train()

    def window(kind):
        tr.criterion = distill if kind == "C" else plain
        tr.teacher = teacher if kind == "C" else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            if kind == "B":
                teacher_forward()
            tr.step(x, target)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for kind in "ABC":                                # every kernel warm
        for _ in range(max(1, args.warmup // args.steps)):
            window(kind)
    assert tr._native_head() is not None
    order = ["A", "B", "A", "C"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    tr.criterion, tr.teacher = plain, None
    by = {k: [v for v, o in zip(ms, order) if o == k] for k in "ABC"}
    a = by["A"]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = {k: [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, o in enumerate(order) if o == k] for k in "BC"}
    r3 = lambda v: round(v, 4)                        # noqa: E731
    med = {k: statistics.median(paired[k]) for k in "BC"}
    res = {
        "what": "training step on a uint8 batch: the plain native step (A), the plain step plus a teacher forward whose logits are "
                "thrown away (B), the distilled step with Trainer(teacher=) (C); same student, teacher and trainer, interleaved windows",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d uint8, Adam; teacher of the same architecture; temperature %g, "
                  "alpha %g, label_smoothing %g, 1000 class weights; %d steps per window, %d rounds of A B A C"
                  % (B, S, S, args.temperature, args.alpha, args.smoothing, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {k: [r3(v) for v in by[k]] for k in "ABC"},
        "ms_per_step_median": {k: r3(statistics.median(by[k])) for k in "ABC"},
        "a_a_scatter_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                           "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(med["B"]), "paired": [r3(v) for v in paired["B"]]},
        "c_minus_a_ms": {"paired_median": r3(med["C"]), "paired": [r3(v) for v in paired["C"]]},
        "c_minus_b_ms": {"from_paired_medians": r3(med["C"] - med["B"]),
                         "note": "the cost of the loss itself; to be read against a_a_scatter_ms"},
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
