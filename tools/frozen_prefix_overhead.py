#!/usr/bin/env python3
"""What a training step with a frozen stage prefix saves against the full step (a measurement helper in the manner of
tools/frozen_bn_overhead.py: not a test, not bench.py, no gate).

BASELINE configs[1] -- MNASNet-1.0, head '512', 1000 classes, bs 256, 224 x 224, Adam, synthetic inputs as bench.py builds them --
ONE model and trainer, timed as INTERLEAVED windows in one process (a difference counts only against the
scatter of the same code in the same call):

  A    trainer.step, nothing frozen                 (the launch lists of the full program)
  Bk   trainer.step after model.freeze(upto=k)      (the backward ends at the first layer of features[k]), k = 2, 4, 6

Window order A B2 A B4 A B6 A ..., so every B window has an A window on either side.  Reported: ms/step of every window, the medians,
the scatter of ADJACENT A windows (what "no difference" looks like here), per k the paired differences against the mean of the two
neighbouring A windows, the launch-list op counts and torch.cuda.max_memory_allocated after a window of each kind run with only
that kind's program alive.  A Bk counts as faster when its median paired difference lies below minus the largest adjacent A-A
difference; for a k that does not, one more step of A and of Bk runs with the engine's profile brackets (Engine.profile_opcodes) on
the weight-gradient and fused-backward opcodes and the launches only Bk contains are listed with their times.

    python tools/frozen_prefix_overhead.py [--steps 40] [--rounds 4] [--out profiles/frozen_prefix_step.json]"""
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

KS = (2, 4, 6)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--rounds", type=int, default=4, help="rounds of A B2 A B4 A B6")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_prefix_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frozen_prefix_overhead.py measures on an MI355X; no GPU here (nothing is estimated on the CPU)")
    from meters_overhead import build
    from mnasnet_pytorch_amd import _lib as L
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, tr = build(dev)
    eng = tr.engine
    g = torch.Generator(device=dev).manual_seed(1234)
    B, S = args.batch, args.size
    x = torch.randn(B, 3, S, S, device=dev, generator=g)
    target = torch.randint(0, 1000, (B,), device=dev, generator=g)

    def window(k, steps=args.steps):
        model.freeze(upto=k)
        assert tr._native_head() is not None and eng.step_stage(eng.first_trainable_step()) == k
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step(x, target)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    kinds = (0,) + KS
    name = lambda k: "B%d" % k if k else "A"          # noqa: E731
    # ---- memory and op counts: every kind alone (its program is the only one alive)
    peak_gb, ops = {}, {}
    for k in kinds:
        eng.reset_programs()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        window(k, 3)
        peak_gb[name(k)] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 3)
        (prog,) = [p for lst in eng.programs.values() for p in lst]
        ops[name(k)] = {"forward": prog.fwd_n, "backward": prog.bwd_all_n, "segments": [st for st, _, _ in prog.bwd_segments]}
        del prog                                      # (or the next kind's peak would include this program)
    eng.reset_programs()
    for k in kinds:                                   # all four programs built, every kernel warm
        window(k)
    order = ([0, KS[0], 0, KS[1], 0, KS[2]] * args.rounds) + [0]
    ms = [window(k) for k in order]
    a = [v for v, k in zip(ms, order) if k == 0]
    a_adj = [abs(p - q) for p, q in zip(a, a[1:])]
    r3 = lambda v: round(v, 4)                        # noqa: E731
    per_k, slow = {}, []
    for k in KS:
        b = [v for v, kk in zip(ms, order) if kk == k]
        paired = [ms[i] - 0.5 * (ms[i - 1] + ms[i + 1]) for i, kk in enumerate(order) if kk == k]
        faster = statistics.median(paired) < -max(a_adj)
        per_k[name(k)] = {"ms_per_step_windows": [r3(v) for v in b], "ms_per_step_median": r3(statistics.median(b)),
                          "minus_a_ms": {"paired_median": r3(statistics.median(paired)), "paired": [r3(v) for v in paired]},
                          "faster_than_a_beyond_a_a_scatter": faster}
        if not faster:
            slow.append(k)
    # ---- a k that is not faster: bracket the candidates and list what only its program launches
    bracket = {L.OP_CONV_WGRAD, L.OP_WGRAD_FINALIZE, L.OP_BWD_POST, L.OP_PW_BWD, L.OP_DW_BWD}
    op_names = {v: n[3:] for n, v in vars(L).items() if n.startswith("OP_") and isinstance(v, int)}
    if slow:
        eng.profile_opcodes = bracket
        prof = {}
        for k in [0] + slow:
            eng.reset_programs()
            window(k, 3)
            times = {}
            for (tag, opcode, ints), t in eng.read_profile():
                if tag == "bwd":
                    times.setdefault((op_names[opcode], tuple(ints)), []).append(t)
            prof[k] = times
        for k in slow:
            only = {key: v for key, v in prof[k].items() if key not in prof[0]}
            gone = {key: v for key, v in prof[0].items() if key not in prof[k] or len(prof[k][key]) < len(v)}
            per_k[name(k)]["profile"] = {
                "bracketed_backward_ms": {"A": r3(sum(sum(v) for v in prof[0].values())), name(k): r3(sum(sum(v) for v in prof[k].values()))},
                "launches_only_in_%s" % name(k): [{"op": key[0], "ints": list(key[1]), "ms": [r3(t) for t in v]} for key, v in sorted(only.items())],
                "launches_of_A_dropped_or_fewer": [{"op": key[0], "ints": list(key[1]), "ms": [r3(t) for t in v]} for key, v in sorted(gone.items())]}
        eng.profile_opcodes = None
        eng.reset_programs()
    model.freeze(upto=0)

    res = {
        "what": "training step with features[:k] frozen (Bk: the backward ends at the first layer of features[k]) against the full step "
                "(A), same model, interleaved windows",
        "config": "MNASNet-1.0 + head '512', 1000 classes, bs %d, %dx%d, Adam, synthetic data; %d steps per window, %d rounds of A B2 A B4 A B6"
                  % (B, S, S, args.steps, args.rounds),
        "gpu": torch.cuda.get_device_name(dev),
        "ms_per_step_windows_A": [r3(v) for v in a],
        "ms_per_step_median_A": r3(statistics.median(a)),
        "a_a_scatter_ms": {"adjacent_max": r3(max(a_adj)), "adjacent_median": r3(statistics.median(a_adj)),
                           "stdev": r3(statistics.pstdev(a)), "min": r3(min(a)), "max": r3(max(a))},
        "per_k": per_k,
        "launch_list_ops": ops,
        "max_memory_allocated_gib": peak_gb,
    }
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
