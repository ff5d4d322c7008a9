#!/usr/bin/env python3
"""What parameter groups, decoupled weight decay and the LAMB trust ratio cost per training step (a measurement helper in the manner
of tools/clip_ema_overhead.py: not a test, not bench.py, no gate and no threshold fixed in advance).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224 uint8 (normalised on the device), synthetic inputs --
ONE model and trainer; FOUR optimizers over its flat buffers (each with its own moments), swapped in between INTERLEAVED windows of one
process (a difference counts only against the scatter of the same code in the same call; a second trainer would
bring its own allocations, and with them differences that are not the optimizer's):

  A  plain Adam                                             (one mnas_adam_step launch over the flat buffer)
  B  Adam with norm_bias_groups                             (one mnas_adam_step_seg call: one update launch, 112 segments)
  C  AdamW with norm_bias_groups and stage_lr_groups        (the same launch, 18 groups, decoupled decay)
  D  LAMB with norm_bias_groups                             (+ the read-only norm pass and the ratio finalize)

Window order A B A C A D ... A, so every B, C and D window has an A window on either side.  Reported: ms/step of every window, the
medians, the scatter of ADJACENT A windows (what "no difference" looks like here), and B - A, C - A, D - A as paired differences
against the mean of the two neighbouring A windows.

Then the update alone: mnas_adam_step_seg over the model's tables against mnas_adam_step over the same element count, on rotating
buffer sets, device events, next to mnas_probe_copy4 moving the update's 7 x 4 bytes per element (rate = bytes moved / time); the
plain launch is repeated to show its own spread.

    python tools/param_groups_overhead.py [--steps 40] [--rounds 4] [--out profiles/param_groups_step.json]"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(dev, **kw):
    from mnasnet_pytorch_amd import FineTuneModelPool, load_model
    from mnasnet_pytorch_amd.train_step import Trainer
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        base = load_model("mnasnet")
    model = FineTuneModelPool(base, "mnasnet", 1000, "512").to(dev).train()
    model.normalize_on_device()
    return Trainer(model, lr=1e-3, **kw)


def update_alone(opt_b, opt_c, opt_d, iters, nsets):
    """the update launches alone, on rotating buffer sets of the model's size"""
    from mnasnet_pytorch_amd import _lib as L
    lib = L.load()
    n = opt_b.flat_p.numel()
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = []
    for _ in range(nsets):
        p, g, m = (torch.randn(n, device="cuda", generator=gen) * 0.1 for _ in range(3))
        sets.append((p, g, m, torch.rand(n, device="cuda", generator=gen) * 1e-2 + 1e-6))

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

    def plain(i):
        p, g, m, v = sets[i]
        L.check(lib.mnas_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 1e-5, 2, 1.0,
                                   L.cur_stream()))

    def seg_of(opt):
        seg = opt._seg_tables()
        tb = seg["tables"]
        trust = opt.trust_ratio is not None
        for k, gr in enumerate(opt.param_groups):
            seg["groups"][k] = L.MnasOptGroup(float(gr["lr"]), float(gr["weight_decay"]), 1 if gr["decoupled"] else 0,
                                              1 if trust and gr["trust"] else 0)
        s = L.MnasOptSegs(segs=seg["segs"].data_ptr(), tiles=seg["tiles"].data_ptr(), groups=seg["groups"], nsegs=len(tb.segs),
                          ntiles=len(tb.tiles), ngroups=len(opt.param_groups), trust_kind=L.TRUST_LAMB if trust else L.TRUST_NONE,
                          tile_partial=L.ptr(seg["partial"]), ratio=L.ptr(seg["ratio"]), trust_coef=1e-3, trust_eps=1e-8)

        def run(i):
            p, g, m, v = sets[i]
            L.check(lib.mnas_adam_step_seg(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0.9, 0.999, 1e-8, 2, 1.0,
                                           ctypes.byref(s), None, L.cur_stream()))
        return run, len(tb.segs), len(tb.tiles)

    nb = (14 * n) // 16384 * 16384                       # the probe moves 2 * nb bytes: the update's 28 bytes per element
    src, dst = (torch.empty(nb, dtype=torch.uint8, device="cuda") for _ in range(2))
    probe = lambda i: L.check(lib.mnas_probe_copy4(src.data_ptr(), dst.data_ptr(), nb, 0, L.cur_stream()))   # noqa: E731
    rows = {}
    plain_us = [timed(plain)]
    probe_us = [timed(probe)]
    for name, opt, passes in (("seg_two_groups", opt_b, 7), ("seg_adamw_18_groups", opt_c, 7), ("seg_lamb", opt_d, 11)):
        run, nsegs, ntiles = seg_of(opt)
        us = timed(run)
        rows[name] = {"us": round(us, 2), "segments": nsegs, "tiles": ntiles, "groups": len(opt.param_groups),
                      "mbytes_moved": round(4 * passes * n / 1e6, 2), "gb_per_s": round(4 * passes * n / (us * 1e-6) / 1e9, 1)}
        plain_us.append(timed(plain))
    probe_us.append(timed(probe))
    pus = statistics.median(plain_us)
    rows["plain_adam_step"] = {"us": round(pus, 2), "us_repeated": [round(v, 2) for v in plain_us],
                               "spread_us": round(max(plain_us) - min(plain_us), 2), "mbytes_moved": round(28 * n / 1e6, 2),
                               "gb_per_s": round(28 * n / (pus * 1e-6) / 1e9, 1)}
    cus = sum(probe_us) / len(probe_us)
    rows["probe_copy4_same_bytes"] = {"us": round(cus, 2), "us_before_after": [round(v, 2) for v in probe_us],
                                      "mbytes_moved": round(2 * nb / 1e6, 2), "gb_per_s": round(2 * nb / (cus * 1e-6) / 1e9, 1)}
    for name in ("seg_two_groups", "seg_adamw_18_groups", "seg_lamb"):
        r = rows[name]
        r["time_per_byte_vs_plain"] = round((r["us"] / r["mbytes_moved"]) / (pus / (28 * n / 1e6)), 3)
        r["us_minus_plain"] = round(r["us"] - pus, 2)
    return {"elements": n, "iters": iters, "rotating_sets": nsets, "launches": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=4, help="rounds of A B A C A D")
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("param_groups_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from mnasnet_pytorch_amd.train_step import norm_bias_groups, stage_lr_groups
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    wd = 1e-5
    nb = lambda m: norm_bias_groups(m, wd)                                                    # noqa: E731
    from mnasnet_pytorch_amd.train_step import FlatAdam
    tr = build(dev, weight_decay=wd)
    every = tr.optimizer._all_params

    def make(groups, **kw):
        return FlatAdam(tr._resolve_groups(groups, every), tr.flat_p, tr.flat_g, lr=1e-3, weight_decay=wd, **kw)

    opts = {"A": tr.optimizer, "B": make(nb),
            "C": make(lambda m: stage_lr_groups(m, 1e-3, 0.8, norm_bias_groups(m, wd)), decoupled_weight_decay=True),
            "D": make(nb, trust_ratio="lamb")}
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)

    def window(kind):
        tr.optimizer = opts[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step(x, target)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for kind in "ABCD":
        for _ in range(max(1, args.warmup // args.steps)):
            window(kind)
    order = ["A", "B", "A", "C", "A", "D"] * args.rounds + ["A"]
    ms = [window(k) for k in order]
    by = {k: [v for v, o in zip(ms, order) if o == k] for k in "ABCD"}
    a = by["A"]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    paired = {k: [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, o in enumerate(order) if o == k] for k in "BCD"}
    r3 = lambda v: round(v, 4)                        # noqa: E731
    tr.optimizer = opts["D"]
    ratios = tr.trust_ratios()
    tr.optimizer = opts["A"]
    res = {
        "what": "training step with parameter groups (B), AdamW over 18 groups (C) and LAMB (D) against the plain Adam step (A): one "
                "trainer, four optimizers over its buffers, interleaved windows; then the update launches alone",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d uint8, synthetic data; weight_decay %g; %d steps per window, %d "
                  "rounds of A B A C A D" % (B, S, S, wd, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "groups": {k: len(o.param_groups) for k, o in opts.items()},
        "seg_calls": {k: o.seg_calls for k, o in opts.items()},
        "ms_per_step_windows": {k: [r3(v) for v in by[k]] for k in "ABCD"},
        "ms_per_step_median": {k: r3(statistics.median(by[k])) for k in "ABCD"},
        "a_a_scatter_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                           "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "minus_a_ms": {k: {"paired_median": r3(statistics.median(paired[k])), "paired": [r3(v) for v in paired[k]]} for k in "BCD"},
        "lamb_trust_ratios": {"tensors": len(ratios), "min": r3(min(ratios.values())), "max": r3(max(ratios.values()))},
        "update_alone": update_alone(opts["B"], opts["C"], opts["D"], args.kernel_iters, 4),
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
