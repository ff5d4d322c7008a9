"""Launch plans as text: every MnasOp of a Program's forward list and backward segments, one line per op, with pointers named by
the tensor they point into.  Programs build on the CPU (the planner only allocates tensors and asks the library host-side
questions), so a change of the planner can be shown to change no launch before it goes near a GPU.

    python tests/golden/make_launch_plan_golden.py                  rewrite tests/golden/launch_plans.txt.gz
    python tests/golden/make_launch_plan_golden.py --dump DIR       one <name>.txt per program (to diff after a mismatch)
    python tests/golden/make_launch_plan_golden.py --dump DIR --device cuda --only NAME [--side-stream] [--profile-bwd]

Line format:  <list> <opcode> i=<15 ints> d=<4 doubles> p=<16 names, trailing empties dropped>
A pointer's name is the tensor whose bytes contain it (+byte offset): module parameter / buffer name, flat_grad, scratch_*,
w_fwd[k] / w_dgrad[k] / w_tconv[k] (index in Engine.convs), in_affine.<f32|u8>, or b<n>:<shape>:<dtype> for the program's own
buffers, numbered by first appearance in the dump (so two plans that alias buffers differently differ).  A null slot is "-"; a pointer
nothing owns is an error.

The fixture is that text gzip-compressed (a third of a megabyte of generated lines otherwise): per program one header line
"== <name> ops=<n> sha256=<digest of its text>", followed, for five programs, by the text itself.  `zcat` shows it."""
import argparse
import bisect
import ctypes
import gzip
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mnasnet_pytorch_amd import Mnasnet              # noqa: E402
from mnasnet_pytorch_amd import _lib as L            # noqa: E402
from mnasnet_pytorch_amd.engine import Engine        # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_plans.txt.gz")
OP_NAMES = {v: k[3:] for k, v in vars(L).items() if k.startswith("OP_") and isinstance(v, int)}
PACK_NAMES = {L.PACK_FWD: "FWD", L.PACK_DGRAD: "DGRAD", L.PACK_DW: "DW", L.PACK_TCONV: "TCONV"}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class _Names:
    """byte ranges -> names"""

    def __init__(self, eng, prog):
        self.ranges = []                 # (start, end, name), name None: a program buffer, named at first use
        self.fresh = {}                  # start -> "b<n>:..."
        self.events = {}
        self.gate = ctypes.addressof(eng.profile_gate)
        named = dict(eng.root.named_parameters())
        named.update(eng.root.named_buffers())
        for name, t in named.items():
            self._add(name, t)
        self._add("flat_grad", eng.flat_grad)
        for name in ("scratch_stats", "scratch_red", "scratch_wgrad", "scratch_wgrad2", "scratch_wgrad3", "scratch_wgrad4"):
            self._add(name, getattr(eng, name))
        for k, ci in enumerate(eng.convs):
            for attr in ("w_fwd", "w_dgrad", "w_tconv"):
                self._add("%s[%d]" % (attr, k), getattr(ci, attr, None))
        for (u8, _dev), t in eng._in_aff.items():
            self._add("in_affine.%s" % ("u8" if u8 else "f32"), t)
        for t in prog.keep:
            self._add(None, t)
        self.ranges.sort(key=lambda r: r[0])
        for (_, e0, n0), (s1, _, n1) in zip(self.ranges, self.ranges[1:]):
            if s1 < e0:
                raise RuntimeError("overlapping tensors %s / %s" % (n0, n1))
        self.starts = [r[0] for r in self.ranges]

    def _add(self, name, t):
        if t is None or t.numel() == 0:
            return
        nbytes = t.numel() * t.element_size()
        self.ranges.append((t.data_ptr(), t.data_ptr() + nbytes,
                            name if name is not None else (tuple(t.shape), str(t.dtype).replace("torch.", ""))))

    def __call__(self, ptr):
        if not ptr:
            return "-"
        k = bisect.bisect_right(self.starts, ptr) - 1
        if k < 0 or ptr >= self.ranges[k][1]:
            raise RuntimeError("pointer %#x belongs to no known tensor" % ptr)
        start, _, name = self.ranges[k]
        if not isinstance(name, str):
            if start not in self.fresh:
                self.fresh[start] = "b%d:%s:%s" % (len(self.fresh), "x".join(map(str, name[0])), name[1])
            name = self.fresh[start]
        return name if ptr == start else "%s+%d" % (name, ptr - start)

    def event(self, h):
        return self.events.setdefault(h, "ev%d" % len(self.events))


def _op_lines(tag, arr, n, names, prog):
    out = []
    for j in range(n):
        o = arr[j]
        if o.opcode in (L.OP_EVENT_RECORD, L.OP_EVENT_WAIT):
            ptrs = [names.event(o.p[0])]
            if o.p[1]:
                if o.p[1] != names.gate:
                    raise RuntimeError("event op with an unknown gate pointer")
                ptrs.append("profile_gate")
            if any(o.p[k] for k in range(2, 16)):
                raise RuntimeError("event op with stray pointers")
        else:
            ptrs = [names(o.p[k]) for k in range(16)]
            while ptrs and ptrs[-1] == "-":
                ptrs.pop()
        out.append("%s %s i=%s d=%s p=%s" % (tag, OP_NAMES[o.opcode], ",".join(str(int(v)) for v in o.i),
                                             ",".join(repr(float(v)) for v in o.d), ",".join(ptrs)))
        if o.opcode == L.OP_PACK_BATCH:
            raw = [t for t in prog.keep if t.data_ptr() == o.p[0]]
            if len(raw) != 1 or raw[0].numel() != int(o.i[0]) * ctypes.sizeof(L.MnasPackDesc):
                raise RuntimeError("PACK_BATCH descriptor array not found among the program's tensors")
            descs = (L.MnasPackDesc * int(o.i[0])).from_buffer_copy(bytes(raw[0].cpu().numpy().tobytes()))
            for d in descs:
                out.append("%s   pack %s Co=%d Ci=%d taps=%d %s -> %s" % (tag, PACK_NAMES[d.kind], d.Co, d.Ci, d.taps, names(d.w), names(d.dst)))
    return out


def dump_program(eng, prog):
    """The text of one program (a list of lines)."""
    names = _Names(eng, prog)
    lines = ["out_shape %s" % (tuple(prog.out_shape),),
             "patch_x %s" % (list(prog.patch_x),), "patch_out %s" % (prog.patch_out,), "patch_gout %s" % (prog.patch_gout,),
             "patch_x_bwd %s" % (prog.patch_x_bwd,), "patch_dx %s" % (prog.patch_dx,),
             "segments %s" % ([st for st, _, _ in prog.bwd_segments],),
             "stage_ranges %s" % (sorted((k, tuple(v)) for k, v in eng.stage_ranges.items()),)]
    lines += _op_lines("fwd", prog.fwd_ops, prog.fwd_n, names, prog)
    for st, arr, n in prog.bwd_segments:
        lines += _op_lines("bwd%d" % st, arr, n, names, prog)
    return lines


def count_ops(lines):
    return sum(1 for ln in lines if ln.startswith(("fwd ", "bwd")) and " i=" in ln)


def digest(lines):
    return hashlib.sha256(("\n".join(lines) + "\n").encode()).hexdigest()


# ---- the configurations ----------------------------------------------------------------------------------------------------------
_TRAIN, _EVAL = True, False
_SHAPES = [("train_256x224x224", (256, 224, 224), _TRAIN), ("train_64x384x512", (64, 384, 512), _TRAIN),
           ("train_2x32x32", (2, 32, 32), _TRAIN), ("eval_256x224x224", (256, 224, 224), _EVAL)]
_SWITCHES = [("merge_post", False, 0.0), ("materialize_dy", False, 0.0), ("use_tconv", False, 0.0), ("dw_fused_k", (3,), 0.0),
             ("pw_recompute_y", False, 0.0), ("dw_masked_g", False, 0.0), ("pw_bwd_segments", 0, 0.0),
             ("pw_split_max_pixels", 10 ** 9, 0.0), ("se_on_load", False, 0.25), ("se_fused_mlp", False, 0.25)]


def configs():
    """[(name, full_text, dict)]: dict = model / subtree / switches / program arguments"""
    out = []
    for ccf in (False, True):
        for se in (0.0, 0.25):
            for sname, shape, training in _SHAPES:
                name = "ccf%d_se%d_%s" % (ccf, 1 if se else 0, sname)
                out.append((name, sname == "train_256x224x224", dict(ccf=ccf, se=se, shape=shape, training=training)))
    out.append(("default_u8_train_256x224x224", False, dict(shape=(256, 224, 224), in_u8=True, norm=True)))
    out.append(("default_unpooled_train_256x224x224", False, dict(shape=(256, 224, 224), pooled=False)))
    out.append(("features3_dx_train_256x56x56", True, dict(shape=(256, 56, 56), subtree=3, need_dx=True, pooled=False)))
    for attr, val, se in _SWITCHES:
        out.append(("default_%s_train_256x224x224" % attr, False, dict(shape=(256, 224, 224), se=se, switches={attr: val})))
    return out


def build_program(cfg, device=torch.device("cpu"), switches=None):
    """(engine, program, model) of one configuration; the model must stay alive as long as the dump is taken"""
    m = Mnasnet(cut_channels_first=cfg.get("ccf", True), se_ratio=cfg.get("se", 0.0)).to(device)
    m.train(cfg.get("training", True))
    root = m.features if cfg.get("subtree") is None else m.features[cfg["subtree"]]
    eng = Engine(root)
    for k, v in dict(cfg.get("switches", {}), **(switches or {})).items():
        if not hasattr(eng, k):
            raise AttributeError("Engine has no switch %s" % k)
        setattr(eng, k, v)
    if cfg.get("norm"):
        eng.set_input_normalization(MEAN, STD)
    eng.ensure_setup(device)
    eng.reset_programs()
    N, H, W = cfg["shape"]
    prog = eng.program(N, H, W, cfg.get("training", True), cfg.get("need_dx", False), cfg.get("pooled", True), cfg.get("in_u8", False))
    return eng, prog, m


def dump_config(cfg, device=torch.device("cpu"), switches=None):
    eng, prog, m = build_program(cfg, device, switches)
    lines = dump_program(eng, prog)
    eng.reset_programs()
    return lines


def fixture_text():
    parts = []
    for name, full, cfg in configs():
        lines = dump_config(cfg)
        parts.append("== %s ops=%d sha256=%s" % (name, count_ops(lines), digest(lines)))
        if full:
            parts += lines
    return "\n".join(parts) + "\n"


def read_fixture(path=FIXTURE):
    """{name: (ops, sha256, lines or None)}"""
    out, cur = {}, None
    with gzip.open(path, "rt") as f:
        for ln in f.read().splitlines():
            if ln.startswith("== "):
                _, name, ops, sha = ln.split(" ")
                cur = []
                out[name] = [int(ops.split("=")[1]), sha.split("=")[1], cur]
            else:
                cur.append(ln)
    return {k: (o, s, lines or None) for k, (o, s, lines) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--only", action="append")
    ap.add_argument("--side-stream", action="store_true")
    ap.add_argument("--profile-bwd", action="store_true", help="profile_opcodes = {OP_PW_BWD, OP_DW_BWD}")
    args = ap.parse_args()
    if not args.dump:
        text = fixture_text()
        with open(FIXTURE, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:      # (no name, no time: reproducible)
            f.write(text.encode())
        print("%s: text sha256 %s (%d bytes)" % (os.path.relpath(FIXTURE, ROOT), hashlib.sha256(text.encode()).hexdigest(), len(text)))
        return
    os.makedirs(args.dump, exist_ok=True)
    switches, suffix = {}, ""
    if args.side_stream:
        switches["use_side_stream"], suffix = True, suffix + ".side"
    if args.profile_bwd:
        switches["profile_opcodes"], suffix = {L.OP_PW_BWD, L.OP_DW_BWD}, suffix + ".prof"
    for name, _, cfg in configs():
        if args.only and name not in args.only:
            continue
        lines = dump_config(cfg, torch.device(args.device), switches)
        with open(os.path.join(args.dump, name + suffix + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        print("%s%s ops=%d sha256=%s" % (name, suffix, count_ops(lines), digest(lines)))


if __name__ == "__main__":
    main()
