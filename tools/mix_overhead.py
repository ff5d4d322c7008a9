#!/usr/bin/env python3
"""What batch mixing and label smoothing cost per training step, and what the mix kernel reaches on its own (a measurement helper in
the manner of tools/clip_ema_overhead.py: not a test, not bench.py, no gate and no threshold fixed in advance).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224, Adam -- on a uint8 batch (normalisation in the
stem's input load).  ONE model and trainer; the criterion is a plain attribute of the trainer, switched between INTERLEAVED windows in
one process (a difference counts only against the scatter of the same code in the same call):

  A  trainer.step(x, target), nn.CrossEntropyLoss()                                    (the plain step)
  B  x, t = DeviceMix(cutmix_alpha=1.0)(x, target); trainer.step(x, t), MixCrossEntropyLoss(0.1)     (CutMix, eps 0.1)
  C  the same with DeviceMix(mixup_alpha=0.2)                                          (Mixup, eps 0.1)

B and C include everything the feature adds to a step: the host draws, the pinned descriptor upload, the mix launch, the gather of
the partner labels and the soft loss kernels.  Window order A B A C A B A C ... A, so every B and C window has an A window on either
side.  Reported: ms/step of every window, the medians, the scatter of ADJACENT A windows (what "no difference" looks like here),
B - A and C - A as paired differences against the mean of the two neighbouring A windows.

Then mnas_img_mix alone (descriptors already on the device; device events; several input / output sets rotate so nothing stays
in the 256 MiB Infinity Cache): copy, Mixup and CutMix (lam 0.5: a centred box of half the area), with the bytes each must move --
x read and out written once, the partner read wholly (Mixup), inside the box rounded out to 16-byte groups (CutMix) or not at all
(copy) -- next to mnas_probe_copy4 moving the same number of bytes per direction in the same process (rate = 2 * bytes / time).

    python tools/mix_overhead.py [--steps 40] [--rounds 6] [--out profiles/mix_step.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402


def kernel_figures(n, h, w, iters, nsets):
    """mnas_img_mix alone against mnas_probe_copy4 on the same number of bytes"""
    from mnasnet_pytorch_amd import _lib as L
    from mnasnet_pytorch_amd.mixing import DeviceMix, MixDraw, cutmix_box
    lib = L.load()
    nb = n * 3 * h * w
    gen = torch.Generator(device="cuda").manual_seed(0)
    xs = [torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
    outs = [torch.empty_like(x) for x in xs]
    box, lam = cutmix_box(h, w, 0.5, h // 2, w // 2)
    partner = lambda k: (k + 1) % n                           # noqa: E731
    kinds = {
        "copy": ([MixDraw(L.IMGM_NONE, k, 65536, (0, 0, 0, 0), 1.0) for k in range(n)], 0.0),
        "mixup": ([MixDraw(L.IMGM_MIXUP, partner(k), 40000, (0, 0, 0, 0), 40000 / 65536.0) for k in range(n)], 1.0),
        "cutmix_half_area": ([MixDraw(L.IMGM_CUTMIX, partner(k), 65536, box, lam) for k in range(n)], None),
    }

    def timed(fn):
        for i in range(nsets):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % nsets)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    rows = {}
    probe_ok = nb % 16384 == 0
    copy_us = []
    if probe_ok:
        copy_us.append(timed(lambda i: L.check(lib.mnas_probe_copy4(xs[i].data_ptr(), outs[i].data_ptr(), nb, 0, L.cur_stream()))))
    for name, (draws, partner_share) in kinds.items():
        arr = DeviceMix.items(draws)
        assert lib.mnas_img_mix_check(arr, n, h, w) == 0
        items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
        us = timed(lambda i: L.check(lib.mnas_img_mix(items.data_ptr(), n, h, w, xs[i].data_ptr(), outs[i].data_ptr(), L.cur_stream())))
        if partner_share is None:                             # the 16-byte groups of a row that touch the box
            y0, x0, y1, x1 = box
            groups = sum(1 for g in range(0, w, 16) if g < x1 and g + 16 > x0) if w % 16 == 0 else None
            partner_share = (y1 - y0) * groups * 16 / float(h * w) if groups is not None else (1.0 - lam)
        by = nb * (2.0 + partner_share)
        rows[name] = {"us": round(us, 2), "mbytes_moved": round(by / 1e6, 2), "gb_per_s": round(by / (us * 1e-6) / 1e9, 1)}
    if probe_ok:
        copy_us.append(timed(lambda i: L.check(lib.mnas_probe_copy4(xs[i].data_ptr(), outs[i].data_ptr(), nb, 0, L.cur_stream()))))
        us = sum(copy_us) / len(copy_us)
        rows["probe_copy4_same_bytes"] = {"us": round(us, 2), "us_before_after": [round(v, 2) for v in copy_us],
                                          "mbytes_moved": round(2 * nb / 1e6, 2), "gb_per_s": round(2 * nb / (us * 1e-6) / 1e9, 1)}
    else:
        rows["probe_copy4_same_bytes"] = "not run: mnas_probe_copy4 needs a multiple of 16384 bytes, the batch has %d" % nb
    return {"batch": [n, 3, h, w], "batch_mbytes": round(nb / 1e6, 2), "iters": iters, "rotating_sets": nsets, "kernels": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=6, help="rounds of A B A C")
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--smoothing", type=float, default=0.1)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--kernel-sets", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mix_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from meters_overhead import build
    from mnasnet_pytorch_amd import DeviceMix, MixCrossEntropyLoss
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, tr = build(dev)
    model.normalize_on_device()
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)
    plain, soft = torch.nn.CrossEntropyLoss(), MixCrossEntropyLoss(args.smoothing)
    mixers = {"B": DeviceMix(cutmix_alpha=1.0), "C": DeviceMix(mixup_alpha=0.2)}
    random.seed(1234)

    def window(kind):
        tr.criterion = plain if kind == "A" else soft
        mix = mixers.get(kind)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            if mix is None:
                tr.step(x, target)
            else:
                tr.step(*mix(x, target))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for kind in "ABC":                                # every kernel warm
        for _ in range(max(1, args.warmup // args.steps)):
            window(kind)
    assert tr._native_head() is not None
    order = ["A", "B", "A", "C"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    tr.criterion = plain
    by = {k: [v for v, o in zip(ms, order) if o == k] for k in "ABC"}
    a = by["A"]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = {k: [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, o in enumerate(order) if o == k] for k in "BC"}
    r3 = lambda v: round(v, 4)                        # noqa: E731
    nb = B * 3 * S * S
    us = lambda nbytes, tbps: round(nbytes / (tbps * 1e12) * 1e6, 2)      # noqa: E731
    res = {
        "what": "training step on a uint8 batch with CutMix + label smoothing (B) and Mixup + label smoothing (C) against the plain "
                "step (A), same model and trainer, interleaved windows; then mnas_img_mix alone against mnas_probe_copy4",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d uint8, Adam; label_smoothing %g, cutmix_alpha 1.0, mixup_alpha "
                  "0.2, one draw per batch; %d steps per window, %d rounds of A B A C" % (B, S, S, args.smoothing, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {k: [r3(v) for v in by[k]] for k in "ABC"},
        "ms_per_step_median": {k: r3(statistics.median(by[k])) for k in "ABC"},
        "a_a_scatter_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                           "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(statistics.median(paired["B"])), "paired": [r3(v) for v in paired["B"]]},
        "c_minus_a_ms": {"paired_median": r3(statistics.median(paired["C"])), "paired": [r3(v) for v in paired["C"]]},
        "traffic_estimate_not_measured": {
            "batch_bytes": nb, "mixup_pass_bytes": 3 * nb,
            "mixup_pass_us_at_4_to_6_TBps": [us(3 * nb, 6), us(3 * nb, 4)],
            "extra_loss_arithmetic": "one fp32 sum over C per row, on the row's max pass",
        },
        "mix_kernel_alone": kernel_figures(B, S, S, args.kernel_iters, args.kernel_sets),
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
