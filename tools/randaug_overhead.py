#!/usr/bin/env python3
"""What RandAugment on the device costs per training step, and what each op's launch reaches on its own (a measurement helper in the
manner of tools/mix_overhead.py: not a test, not bench.py, no gate and no threshold fixed in advance).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224, Adam -- on a uint8 batch (normalisation in the
stem's input load).  ONE model and trainer, INTERLEAVED windows in one process (a difference counts only against
the scatter of the same code in the same call):

  A  trainer.step(x, target)                                         (the plain step)
  B  trainer.step(DeviceRandAugment(2, 9)(x), target)                (two ops per image at magnitude 9 of 31)

B includes everything the feature adds to a step: the host draws, the descriptor array, the pinned upload, the workspace and up to
two statistics and two apply launches.  Window order A B A B ... A, so every B window has an A window on either side.  Reported:
ms/step of every window, the medians, the scatter of ADJACENT A windows (what "no difference" looks like here), and B - A as paired
differences against the mean of the two neighbouring A windows.

Then mnas_img_aug alone (descriptors already on the device; device events; several input / output sets rotate so nothing stays in
the 256 MiB Infinity Cache): one batch per op in which every image carries that op alone -- one apply launch, or for CONTRAST,
AUTOCONTRAST and EQUALIZE the statistics launch and the apply launch together (mnas_img_aug issues the pair; they are not timed
apart) -- and a seeded RandAugment batch, with the bytes each must move (the batch read and written once; read twice with a
statistics launch), next to mnas_probe_copy4 moving the same batch in the same process (rate = 2 * bytes / time).  A launch that
takes more than three times the copy probe's time for the bytes it moves is listed with what it does beyond moving bytes.

    python tools/randaug_overhead.py [--steps 40] [--rounds 6] [--out profiles/randaug_step.json]"""
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

# what a launch does per pixel beyond one 16-byte load and store per 16 bytes (stated from the kernel's code, not measured)
BEYOND_COPY = {
    "affine": "three single-byte gathers per pixel from an address computed per pixel; neighbouring lanes' sources are not contiguous under a rotation",
    "sharpness": "per plane and 16 pixels two more 16-byte loads (the rows above and below) and up to six single bytes (the columns either "
                 "side), 18 column sums, and per byte a division by 26 and an fp32 blend",
    "statistics": "a second pass over the batch with three LDS atomic increments per pixel (one histogram per wave), then a 256-step "
                  "serial scan per channel in every workgroup of the apply launch",
    "contrast": "a second pass over the batch for the grey sum",
}


def kernel_figures(n, h, w, iters, nsets):
    """mnas_img_aug, one op per image, against mnas_probe_copy4 on the same batch"""
    from mnasnet_pytorch_amd import DeviceRandAugment
    from mnasnet_pytorch_amd import _lib as L
    from mnasnet_pytorch_amd import augment as AU
    lib = L.load()
    nb = n * 3 * h * w
    gen = torch.Generator(device="cuda").manual_seed(0)
    xs = [torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(nsets)]
    outs = [torch.empty_like(x) for x in xs]
    kinds = {
        "identity": ((L.IMGA_IDENTITY, 0.0, ()), None),
        "affine_rotate_9": ((L.IMGA_AFFINE, 0.0, AU.affine_args(AU.rotate_matrix(9.0, h, w))), "affine"),
        "affine_shear_x": ((L.IMGA_AFFINE, 0.0, AU.affine_args((1, 0.09, 0, 0, 1, 0))), "affine"),
        "affine_translate_x": ((L.IMGA_AFFINE, 0.0, AU.affine_args((1, 0, 30, 0, 1, 0))), "affine"),
        "brightness": ((L.IMGA_BRIGHTNESS, 1.27, ()), None),
        "color": ((L.IMGA_COLOR, 1.27, ()), None),
        "contrast": ((L.IMGA_CONTRAST, 1.27, ()), "contrast"),
        "sharpness": ((L.IMGA_SHARPNESS, 1.27, ()), "sharpness"),
        "posterize": ((L.IMGA_POSTERIZE, 0.0, (7,)), None),
        "solarize": ((L.IMGA_SOLARIZE, 0.0, (179,)), None),
        "invert": ((L.IMGA_INVERT, 0.0, ()), None),
        "autocontrast": ((L.IMGA_AUTOCONTRAST, 0.0, ()), "statistics"),
        "equalize": ((L.IMGA_EQUALIZE, 0.0, ()), "statistics"),
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

    def run_rows(rows):
        arr = AU.aug_items(rows)
        assert lib.mnas_img_aug_check(arr, n, h, w) == 0
        max_ops, stages = AU.aug_plan(arr, n)
        items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
        nws = lib.mnas_img_aug_workspace_bytes(n, h, w, max_ops, int(stages != 0))
        ws = torch.empty(max(16, nws), dtype=torch.uint8, device="cuda")
        launches = max(1, max_ops) + bin(stages).count("1")
        us = timed(lambda i: L.check(lib.mnas_img_aug(items.data_ptr(), n, h, w, max_ops, stages, 0, xs[i].data_ptr(), outs[i].data_ptr(),
                                                      ws.data_ptr(), L.cur_stream())))
        return us, launches

    probe = lambda: timed(lambda i: L.check(lib.mnas_probe_copy4(xs[i].data_ptr(), outs[i].data_ptr(), nb, 0, L.cur_stream())))  # noqa: E731
    probe_ok = nb % 16384 == 0
    copy_us = [probe()] if probe_ok else []
    rows = {}
    for name, (op, beyond) in kinds.items():
        us, launches = run_rows([[op]] * n)
        by = nb * (2.0 + (launches - 1))
        rows[name] = {"us": round(us, 2), "launches": launches, "mbytes_moved": round(by / 1e6, 2),
                      "gb_per_s": round(by / (us * 1e-6) / 1e9, 1), "beyond_copy": beyond}
    random.seed(1234)
    ra_rows = [[(o.op, o.factor, o.args) for o in r] for r in DeviceRandAugment(2, 9).describe(n, (h, w))]
    us, launches = run_rows(ra_rows)
    rows["randaugment_2_9_seed_1234"] = {"us": round(us, 2), "launches": launches}
    if probe_ok:
        copy_us.append(probe())
        cus = sum(copy_us) / len(copy_us)
        rows["probe_copy4_same_batch"] = {"us": round(cus, 2), "us_before_after": [round(v, 2) for v in copy_us],
                                          "mbytes_moved": round(2 * nb / 1e6, 2), "gb_per_s": round(2 * nb / (cus * 1e-6) / 1e9, 1)}
        slow = {}
        for name, r in rows.items():
            if "mbytes_moved" in r and name != "probe_copy4_same_batch":
                ratio = (r["us"] / r["mbytes_moved"]) / (cus / (2 * nb / 1e6))
                r["time_per_byte_vs_probe"] = round(ratio, 2)
                if ratio > 3.0:
                    slow[name] = BEYOND_COPY.get(r["beyond_copy"], "nothing beyond the copy in the code: unexplained")
        rows["more_than_3x_the_probe_per_byte"] = slow
    else:
        rows["probe_copy4_same_batch"] = "not run: mnas_probe_copy4 needs a multiple of 16384 bytes, the batch has %d" % nb
    return {"batch": [n, 3, h, w], "batch_mbytes": round(nb / 1e6, 2), "iters": iters, "rotating_sets": nsets, "kernels": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=6, help="rounds of A B")
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--kernel-iters", type=int, default=100)
    ap.add_argument("--kernel-sets", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randaug_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("randaug_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from meters_overhead import build
    from mnasnet_pytorch_amd import DeviceRandAugment
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, tr = build(dev)
    model.normalize_on_device()
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)
    ra = DeviceRandAugment(2, 9)
    random.seed(1234)

    def window(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step(x if kind == "A" else ra(x), target)
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
    # the host side of one call, alone: draws and descriptor array (no GPU work)
    t0 = time.perf_counter()
    for _ in range(20):
        from mnasnet_pytorch_amd.augment import aug_items
        aug_items(ra.describe(B, (S, S)))
    host_ms = (time.perf_counter() - t0) / 20 * 1e3
    r3 = lambda v: round(v, 4)                        # noqa: E731
    res = {
        "what": "training step on a uint8 batch under DeviceRandAugment(2, 9) (B) against the plain step (A), same model and trainer, "
                "interleaved windows; then mnas_img_aug alone, one op per image, against mnas_probe_copy4",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d uint8, Adam; num_ops 2, magnitude 9 of 31; %d steps per window, "
                  "%d rounds of A B" % (B, S, S, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows": {k: [r3(v) for v in by[k]] for k in "AB"},
        "ms_per_step_median": {k: r3(statistics.median(by[k])) for k in "AB"},
        "a_a_scatter_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                           "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "b_minus_a_ms": {"paired_median": r3(statistics.median(paired)), "paired": [r3(v) for v in paired]},
        "host_draws_and_descriptors_ms_per_call": r3(host_ms),
        "aug_kernels_alone": kernel_figures(B, S, S, args.kernel_iters, args.kernel_sets),
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
