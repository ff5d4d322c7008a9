#!/usr/bin/env python3
"""What Random Erasing on the device costs per training step, and what the erase launch takes on its own (a measurement helper in the
manner of tools/mix_overhead.py: not a test, not bench.py, no gate and no threshold fixed in advance).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224, Adam -- on a uint8 batch (normalisation in the
stem's input load).  ONE model and trainer, INTERLEAVED windows in one process (a difference counts only against
the scatter of the same code in the same call):

  A  trainer.step(x, target)                                                     (the plain step)
  B  trainer.step(DeviceRandomErasing(0.25, mode="pixel")(x), target)            (the recipe's draw)

B includes everything the feature adds to a step: the host draws, the descriptor array, the pinned upload and the launch.  The erase is
in place, so the batch of the B windows gathers noise boxes as the run goes on; the step's time does not depend on the bytes.  Window
order A B A B ... A, so every B window has an A window on either side.  Reported: ms/step of every window, the medians, the scatter
of ADJACENT A windows (what "no difference" looks like here), and B - A as paired differences against the mean of the two
neighbouring A windows.

Then mnas_img_erase alone (descriptors already on the device; device events; several batches rotate so nothing stays in the 256 MiB
Infinity Cache): one seeded draw of the recipe as "pixel" (NOISE) and as "const", and the worst case, a full-image NOISE box on every
image, each with the bytes it writes, next to mnas_probe_copy4 moving the whole batch once in the same process.

    python tools/erase_overhead.py [--steps 40] [--rounds 6] [--out profiles/erase_step.json]"""
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
    """mnas_img_erase alone against mnas_probe_copy4 on the whole batch"""
    from mnasnet_pytorch_amd import DeviceRandomErasing
    from mnasnet_pytorch_amd import _lib as L
    from mnasnet_pytorch_amd.erasing import EraseBox, _device_table
    lib = L.load()
    nb = n * 3 * h * w
    gen = torch.Generator(device="cuda").manual_seed(0)
    xs = [torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
    outs = [torch.empty_like(x) for x in xs]
    er = DeviceRandomErasing(0.25, mode="pixel")
    table = _device_table(er.mean, er.std, xs[0].device)
    random.seed(4321)
    recipe, seed = er.describe(n, h, w)
    kinds = {
        "pixel_recipe_draw": recipe,
        "const_recipe_draw": [[b._replace(mode=L.IMGE_CONST, fill=(124, 116, 104)) for b in boxes] for boxes in recipe],
        "pixel_full_image_every_image": [[EraseBox(L.IMGE_NOISE, (0, 0, h, w), (0, 0, 0))] for _ in range(n)],
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
    empty_us = timed(lambda i: L.check(lib.mnas_probe_empty(1, 256, L.cur_stream())))
    for name, draws in kinds.items():
        arr = DeviceRandomErasing.items(draws, 0)
        assert lib.mnas_img_erase_check(arr, n, h, w) == 0
        items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
        us = timed(lambda i: L.check(lib.mnas_img_erase(items.data_ptr(), n, h, w, xs[i].data_ptr(), table.data_ptr(), seed, 0,
                                                        L.cur_stream())))
        written = 3 * sum((b.box[2] - b.box[0]) * (b.box[3] - b.box[1]) for boxes in draws for b in boxes[:1])
        rows[name] = {"us": round(us, 2), "images_erased": sum(1 for boxes in draws if boxes), "mbytes_written": round(written / 1e6, 3),
                      "share_of_batch": round(written / nb, 4), "gb_per_s_written": round(written / (us * 1e-6) / 1e9, 1)}
    if probe_ok:
        copy_us.append(timed(lambda i: L.check(lib.mnas_probe_copy4(xs[i].data_ptr(), outs[i].data_ptr(), nb, 0, L.cur_stream()))))
        us = sum(copy_us) / len(copy_us)
        rows["probe_copy4_whole_batch"] = {"us": round(us, 2), "us_before_after": [round(v, 2) for v in copy_us],
                                           "mbytes_moved": round(2 * nb / 1e6, 2), "gb_per_s": round(2 * nb / (us * 1e-6) / 1e9, 1)}
    else:
        rows["probe_copy4_whole_batch"] = "not run: mnas_probe_copy4 needs a multiple of 16384 bytes, the batch has %d" % nb
    rows["probe_empty_launch"] = {"us": round(empty_us, 2)}
    return {"batch": [n, 3, h, w], "batch_mbytes": round(nb / 1e6, 2), "iters": iters, "rotating_sets": nsets,
            "timing": "back-to-back launches in one stream between two device events, per launch", "kernels": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=6, help="rounds of A B")
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--kernel-sets", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "erase_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("erase_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from meters_overhead import build
    from mnasnet_pytorch_amd import DeviceRandomErasing
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, tr = build(dev)
    model.normalize_on_device()
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)
    er = DeviceRandomErasing(0.25, mode="pixel")
    random.seed(1234)

    def window(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step(x if kind == "A" else er(x), target)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for kind in "AB":                                 # every kernel warm
        for _ in range(max(1, args.warmup // args.steps)):
            window(kind)
    assert tr._native_head() is not None
    order = ["A", "B"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    by = {k: [v for v, o in zip(ms, order) if o == k] for k in "AB"}
    a = by["A"]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, o in enumerate(order) if o == "B"]
    # the host side of one call, alone: draws and descriptor array (no GPU work); and the share of the batch the draws erase
    t0 = time.perf_counter()
    area = []
    for _ in range(20):
        draws, _ = er.describe(B, S, S)
        DeviceRandomErasing.items(draws, 0)
        area.append(sum((b.box[2] - b.box[0]) * (b.box[3] - b.box[1]) for boxes in draws for b in boxes) / float(B * S * S))
    host_ms = (time.perf_counter() - t0) / 20 * 1e3
    r3 = lambda v: round(v, 4)                        # noqa: E731
    nb = B * 3 * S * S
    res = {
        "what": "training step on a uint8 batch under DeviceRandomErasing(0.25, mode='pixel') (B) against the plain step (A), same model "
                "and trainer, interleaved windows; then mnas_img_erase alone against mnas_probe_copy4 moving the batch once",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d uint8, Adam; prob 0.25, area 0.02..1/3, aspect 0.3..1/0.3, one box; "
                  "%d steps per window, %d rounds of A B" % (B, S, S, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {k: [r3(v) for v in by[k]] for k in "AB"},
        "ms_per_step_median": {k: r3(statistics.median(by[k])) for k in "AB"},
        "a_a_scatter_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                           "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(statistics.median(paired)), "paired": [r3(v) for v in paired]},
        "host_draws_and_descriptors_ms_per_call": r3(host_ms),
        "share_of_batch_erased_mean_of_20_draws": r3(statistics.mean(area)),
        "traffic_estimate_not_measured": {"batch_bytes": nb, "written_bytes_at_prob_0.25_and_mean_area_0.18": int(nb * 0.25 * 0.18)},
        "erase_kernel_alone": kernel_figures(B, S, S, args.kernel_iters, args.kernel_sets),
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
