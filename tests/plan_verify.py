"""Static verifier of a Program's launch lists (host code only): walks the forward list and the backward segments in order with the
access model of tests/plan_access.py and reports what would make the lists wrong whatever the kernels do right.

    view = PlanView(prog)                      # copies of the op arrays (a test may edit them) and of the patch records
    findings = verify(eng, view)               # [] = nothing found

Checks (Finding.kind):
  patch      a patch_* record points at a slot whose mode is not the one the run-time pointer needs (x, gout, x_bwd: read; out, dx:
             write), or bwd_all is not the concatenation of the segments.  With a patch finding the walk is not run: the lists
             cannot be given their run-time pointers.
  extent     a declared range does not lie inside the tensor that owns its first byte.
  order      two accesses to overlapping bytes, at least one a write, that happens-before does not order.  Happens-before: list order
             per stream (i[14]) and record -> wait of each event.  After the last op the consumer of the step (the optimizer, the
             caller) reads flat_grad, the output and dx on stream 0: a write that is not joined by then is reported at the writer.
  undefined  a byte is read that no ordered-earlier op of this forward + backward wrote and that is not defined at start.
  writer     a read of an engine scratch table does not see exactly what ONE producer launch wrote through one slot: rows partly
             from its producer and partly from an older op, a different extent than the producer's (an nparts / nsplit mismatch),
             or rows another launch has already reduced (every table has one consumer: a stale table of the right shape).
  liveness   the backward reads a byte of a program buffer that the forward wrote and a backward op has overwritten since.
  cover      flat_grad: a write that is not exactly one parameter's range (reported at the op), or a parameter whose range is the
             target of another number of launches than it has applications behind first_trainable (reported at list "params").

Defined at start: DEFINED_AT_START below.  One finding per (list, op, slot); its kinds are joined with '+'."""
import bisect
from collections import namedtuple

import torch

import make_launch_plan_golden as G
import plan_access as A
from mnasnet_pytorch_amd import _lib as L

Finding = namedtuple("Finding", "list index opcode slot kind detail")

# What holds defined bytes before the first op of a forward, and why:
DEFINED_AT_START = {
    "parameters and module buffers": "the model's state (running statistics and num_batches_tracked are read-modify-write)",
    "flat_grad": "Engine.prepare_grads zeroes it or keeps the accumulated gradients; every gradient launch adds into it",
    "in_affine.*": "Engine.input_affine fills the table when the normalisation is set",
    "descriptor arrays": "LaunchPlan uploads them when the plan is built",
    "x, gout": "the caller's tensors behind patch_x / patch_x_bwd and patch_gout",
}
# LaunchPlan._bnbuf allocates the coefficient blocks with torch.zeros.  They are treated as UNDEFINED here: no plan reads a row
# before a launch of the same step wrote it (rows 0, 1, 5, 6: the forward finalize or mnas_bn_frozen_tables; rows 2..4: the backward
# finalize; row 7: never read), so nothing relies on the zero and this set is empty.
ZEROED_AND_NEEDED = {}

_IO = ("x", "out", "gout", "dx")
_START = -1          # writer id of bytes defined at start


def copy_ops(arr, n):
    return [L.MnasOp.from_buffer_copy(arr[j]) for j in range(n)]


class PlanView:
    """Editable copies of a Program's lists and patch records."""

    def __init__(self, prog):
        self.prog = prog
        self.fwd = copy_ops(prog.fwd_ops, prog.fwd_n)
        self.segments = [(st, copy_ops(arr, n)) for st, arr, n in prog.bwd_segments]
        self.bwd_all = copy_ops(prog.bwd_all, prog.bwd_all_n) if prog.bwd_segments else []
        self.patch_x, self.patch_out = list(prog.patch_x), prog.patch_out
        self.patch_gout, self.patch_x_bwd, self.patch_dx = prog.patch_gout, prog.patch_x_bwd, prog.patch_dx
        self.extra_owners = {}          # name -> tensor: owners a test adds (a replaced scratch)

    def lists(self):
        """[(list name, ops)] in launch order"""
        return [("fwd", self.fwd)] + [("bwd%d" % st, ops) for st, ops in self.segments]

    def seg(self, stage):
        return next(ops for st, ops in self.segments if st == stage)


def slot_name(opcode, k):
    return L.OP_SLOTS[opcode][2][k]


def _merge(ranges):
    out = []
    for a, b in sorted(ranges):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(r) for r in out]


class _Owners:
    """Who owns a byte: make_launch_plan_golden._Names plus the run-time tensors and what a test adds."""

    def __init__(self, eng, prog, extra):
        names = G._Names(eng, prog)
        for name, t in extra.items():
            names._add(name, t)
        names.ranges.sort(key=lambda r: r[0])
        names.starts = [r[0] for r in names.ranges]
        self.ranges, self.starts = names.ranges, names.starts
        self.tensors = {t.data_ptr(): t for t in prog.keep}
        self.param_names = set(dict(eng.root.named_parameters())) | set(dict(eng.root.named_buffers()))
        self.descs = {t.data_ptr() for t in prog.keep if t.dtype == torch.uint8}

    def find(self, ptr):
        k = bisect.bisect_right(self.starts, ptr) - 1
        if k < 0 or ptr >= self.ranges[k][1]:
            return None
        return k

    def label(self, k):
        start, end, name = self.ranges[k]
        return name if isinstance(name, str) else "buffer %s %s" % ("x".join(map(str, name[0])), name[1])

    def defined_at_start(self, k):
        start, _, name = self.ranges[k]
        if not isinstance(name, str):
            return start in self.descs
        return name in self.param_names or name == "flat_grad" or name.startswith("in_affine.") or name in ("x", "gout")

    def is_scratch(self, k):
        name = self.ranges[k][2]
        return isinstance(name, str) and name.startswith("scratch_")

    def peek(self, ptr, n):
        k = self.find(ptr)
        t = self.tensors.get(self.ranges[k][0]) if k is not None else None
        if t is None:
            raise RuntimeError("descriptor array %#x is no tensor of the program" % ptr)
        off = ptr - t.data_ptr()
        return bytes(t.cpu().numpy().tobytes()[off:off + n])


class _Seg:
    __slots__ = ("a", "b", "writer", "readers", "fwd_writer")

    def __init__(self, a, b, writer, readers=(), fwd_writer=None):
        self.a, self.b, self.writer, self.readers, self.fwd_writer = a, b, writer, list(readers), fwd_writer


class _Map:
    """the bytes of one tensor as segments with one history each"""

    def __init__(self, a, b, writer):
        self.segs = [_Seg(a, b, writer)]

    def cut(self, a, b):
        """the segments covering [a, b), split at its ends"""
        out, new = [], []
        for s in self.segs:
            if s.b <= a or s.a >= b:
                new.append(s)
                continue
            if s.a < a:
                new.append(_Seg(s.a, a, s.writer, s.readers, s.fwd_writer))
            mid = _Seg(max(s.a, a), min(s.b, b), s.writer, s.readers, s.fwd_writer)
            new.append(mid)
            out.append(mid)
            if s.b > b:
                new.append(_Seg(b, s.b, s.writer, s.readers, s.fwd_writer))
        self.segs = new
        return out

    def compact(self):
        new = []
        for s in self.segs:
            p = new[-1] if new else None
            if p is not None and p.b == s.a and p.writer == s.writer and p.readers == s.readers and p.fwd_writer == s.fwd_writer:
                p.b = s.b
            else:
                new.append(s)
        self.segs = new


def io_tensors(eng, prog):
    """CPU stand-ins for the tensors the run-time half patches in"""
    N, H, W = prog.N, prog.H, prog.W
    x = torch.empty((N, prog.in_channels, H, W), dtype=torch.uint8 if prog.in_u8 else torch.float32)
    return {"x": x, "out": torch.empty(prog.out_shape, dtype=torch.float32), "gout": torch.empty(prog.out_shape, dtype=torch.float32),
            "dx": torch.empty((N, prog.in_channels, H, W), dtype=torch.float32)}


def _slot_modes(o, lib, peek, k):
    name = slot_name(o.opcode, k)
    return name, {m for n_, m, _, _ in A.op_accesses(o, lib, peek) if n_ == name}


def check_patches(eng, view, io):
    """The patch records against the modes of the slots they name; bwd_all against the segments.  Applies the patches to the view."""
    lib, prog, out = eng.lib, view.prog, []
    raw_all = [bytes(o) for o in view.bwd_all]
    raw_segs = [bytes(o) for _, ops in view.segments for o in ops]
    if view.segments and raw_all != raw_segs:
        k = next((k for k, (a, b) in enumerate(zip(raw_all, raw_segs)) if a != b), min(len(raw_all), len(raw_segs)))
        out.append(Finding("bwd_all", k, "", "", "patch", "bwd_all is not the concatenation of the segments from op %d on" % k))
    owners = _Owners(eng, prog, {})
    seg_off, k = {}, 0
    for st, ops in view.segments:
        seg_off["bwd%d" % st] = k
        k += len(ops)

    def one(what, lst, ops, j, k, tensor, want):
        if not 0 <= j < len(ops) or slot_name(ops[j].opcode, k) is None:
            out.append(Finding(lst, j, "", "", "patch", "%s names no slot" % what))
            return
        ops[j].p[k] = tensor.data_ptr()
        if lst in seg_off and seg_off[lst] + j < len(view.bwd_all):        # (Program.run_backward patches both)
            view.bwd_all[seg_off[lst] + j].p[k] = tensor.data_ptr()
        name, modes = _slot_modes(ops[j], lib, owners.peek, k)
        if modes != {want}:
            out.append(Finding(lst, j, G.OP_NAMES[ops[j].opcode], name, "patch",
                               "%s needs a slot that is %s; the model says %s" % (what, want, sorted(modes) or "untouched")))

    for j, k in view.patch_x:
        one("patch_x", "fwd", view.fwd, j, k, io["x"], A.R)
    one("patch_out", "fwd", view.fwd, view.patch_out[0], view.patch_out[1], io["out"], A.W)
    for what, rec, t, want in (("patch_gout", view.patch_gout, io["gout"], A.R), ("patch_x_bwd", view.patch_x_bwd, io["x"], A.R),
                               ("patch_dx", view.patch_dx, io["dx"], A.W)):
        if rec is not None:
            st, j, k = rec
            one(what, "bwd%d" % st, view.seg(st), j, k, t, want)
    return out


def applications(eng, first_trainable):
    """{id(owner): forward applications of the ConvBlock / SqueezeExcite module in the steps the backward covers}"""
    count = {}
    for si, (op, m, _) in enumerate(eng.steps):
        if si < first_trainable:
            continue
        for cb in ([m] if op == "conv" else m):
            count[id(eng.info[id(cb)])] = count.get(id(eng.info[id(cb)]), 0) + 1
        if op == "block" and id(m[0]) in eng.se_info:
            se = eng.se_info[id(m[0])]
            count[id(se)] = count.get(id(se), 0) + 1
    return count


def expected_cover(eng, prog):
    """{(first byte, bytes) of a parameter's range in flat_grad: (parameter label, launches that must target it)}.
    A conv bias under batch statistics gets no launch: the planner leaves its gradient at exactly zero (engine.py: BatchNorm cancels
    the bias); under frozen statistics the finalize adds s * S1 once per application."""
    has_bwd = prog.training and prog.first_trainable < len(eng.steps)
    apps = applications(eng, prog.first_trainable) if has_bwd else {}
    names = {id(p): n for n, p in eng.root.named_parameters()}
    out, base = {}, eng.flat_grad.data_ptr()
    for owner in eng.param_owners:
        for j, p in enumerate(owner.params):
            off, numel = owner.gslice[j]
            n = apps.get(id(owner), 0)
            if owner in eng.convs and j == 1 and not prog.frozen_bn:
                n = 0
            out[(base + 4 * off, 4 * numel)] = (names.get(id(p), "?"), n)
    return out


def verify(eng, view):
    """All findings of one plan view (see the module docstring)."""
    prog, lib = view.prog, eng.lib
    io = io_tensors(eng, prog)
    found = check_patches(eng, view, io)
    if found:
        return found
    extra = dict(io)
    extra.update(view.extra_owners)
    owners = _Owners(eng, prog, extra)
    maps = {k: _Map(s, e, _START if owners.defined_at_start(k) else None) for k, (s, e, _) in enumerate(owners.ranges)}
    acc = {}            # (list, index, slot) -> [kinds, details, opcode]

    def report(lst, j, o, slot, kind, detail):
        e = acc.setdefault((lst, j, slot), [[], [], G.OP_NAMES.get(o.opcode, "") if o is not None else ""])
        if kind not in e[0]:
            e[0].append(kind)
            e[1].append(detail)

    # ---- happens-before: vector clocks over the two streams
    ops_seq = []         # op id -> (list, index, op, stream, clock)
    clock = [[0, 0], [0, 0]]
    events = {}

    def hb(a, b_clock):
        _, _, _, s, ca = ops_seq[a]
        return ca[s] <= b_clock[s]

    writes = {}          # (op id, slot, owner) -> written ranges
    consumed = {}        # (writer op id, owner, rows) -> (op id, slot) of the first reader of a scratch table
    cover = expected_cover(eng, prog)
    cover_hits = {k: 0 for k in cover}
    flat_k = owners.find(eng.flat_grad.data_ptr())
    in_bwd = False

    def where(opid):
        lst, j, o, _, _ = ops_seq[opid]
        return "%s[%d] %s" % (lst, j, G.OP_NAMES[o.opcode])

    def access(opid, lst, j, o, b_clock, slot, mode, start, n, reads_by_owner):
        k = owners.find(start)
        if k is None:
            report(lst, j, o, slot, "extent", "%#x belongs to no tensor" % start)
            return
        s0, e0, _ = owners.ranges[k]
        end = start + n
        if end > e0:
            report(lst, j, o, slot, "extent", "%d bytes from offset %d of %s, which has %d" % (n, start - s0, owners.label(k), e0 - s0))
            end = e0
        m = maps[k]
        for seg in m.cut(start, end):
            if mode in (A.R, A.RW):
                if seg.writer is None:
                    report(lst, j, o, slot, "undefined", "reads bytes %d.. of %s that nothing has written" % (seg.a - s0, owners.label(k)))
                elif seg.writer != _START and not hb(seg.writer, b_clock):
                    report(lst, j, o, slot, "order", "reads %s while %s writes it" % (owners.label(k), where(seg.writer)))
                if in_bwd and seg.fwd_writer is not None and not owners.is_scratch(k):
                    report(lst, j, o, slot, "liveness", "%s was written by %s and overwritten by %s before this read" %
                           (owners.label(k), where(seg.fwd_writer), where(seg.writer)))
                if mode == A.R:
                    reads_by_owner.setdefault((slot, k), []).append((seg.a, seg.b, seg.writer))
                    seg.readers.append(opid)
            if mode in (A.W, A.RW):
                if seg.writer not in (None, _START) and not hb(seg.writer, b_clock):
                    report(lst, j, o, slot, "order", "writes %s while %s writes it" % (owners.label(k), where(seg.writer)))
                for r in seg.readers:
                    if r != opid and not hb(r, b_clock):
                        report(lst, j, o, slot, "order", "writes %s while %s reads it" % (owners.label(k), where(r)))
                if in_bwd and seg.fwd_writer is None and seg.writer not in (None, _START) and ops_seq[seg.writer][0] == "fwd":
                    seg.fwd_writer = seg.writer
                seg.writer, seg.readers = opid, []
                writes.setdefault((opid, slot, k), []).append((seg.a, seg.b))
        m.compact()
        if k == flat_k and mode in (A.W, A.RW):
            if (start, n) in cover_hits:
                cover_hits[(start, n)] += 1
            else:
                report(lst, j, o, slot, "cover", "writes flat_grad[%d:%d], which is no parameter's range" % ((start - s0) // 4, (end - s0) // 4))
        elif k == flat_k:
            report(lst, j, o, slot, "cover", "reads flat_grad without writing it")

    for lst, ops in view.lists():
        in_bwd = lst != "fwd"
        for j, o in enumerate(ops):
            s = int(o.i[L.OP_STREAM_SLOT])
            if s not in (0, 1):
                report(lst, j, o, "", "order", "stream %d" % s)
                continue
            clock[s][s] += 1
            if o.opcode == L.OP_EVENT_WAIT:
                ev = events.get(o.p[0])
                if ev is None:
                    report(lst, j, o, "event", "order", "waits for an event nobody has recorded")
                else:
                    clock[s] = [max(a, b) for a, b in zip(clock[s], ev)]
            my = list(clock[s])
            opid = len(ops_seq)
            ops_seq.append((lst, j, o, s, my))
            if o.opcode == L.OP_EVENT_RECORD:
                if not o.p[1]:              # (a gated record brackets a launch for the profiler: nobody waits for it)
                    events[o.p[0]] = my
                continue
            if o.opcode == L.OP_EVENT_WAIT:
                continue
            accs = A.op_accesses(o, lib, owners.peek)
            reads_by_owner = {}
            for phase in ((A.R, A.RW), (A.W,)):
                for slot, mode, start, n in accs:
                    if mode in phase:
                        access(opid, lst, j, o, my, slot, mode, start, n, reads_by_owner)
            # ---- what a finalize reads of a scratch table is what one producer wrote, no more and no less
            for (slot, k), segs in reads_by_owner.items():
                if not owners.is_scratch(k):
                    continue
                ws = {w for _, _, w in segs}
                if None in ws or _START in ws:
                    continue                # (reported as undefined)
                got = _merge([(a, b) for a, b, _ in segs])
                if len(ws) > 1:
                    report(lst, j, o, slot, "writer", "rows of %s partly from %s" % (owners.label(k), " and partly from ".join(where(w) for w in sorted(ws))))
                    continue
                w = ws.pop()
                slots_w = {sl: _merge(r) for (op_, sl, k_), r in writes.items() if op_ == w and k_ == k}
                first = consumed.setdefault((w, k, tuple(got)), (opid, slot))
                if first != (opid, slot):
                    # (every table here has one consumer: a second reader of the same rows sees a stale table of the right shape)
                    report(lst, j, o, slot, "writer", "reads the rows of %s that %s wrote and %s has already reduced" %
                           (owners.label(k), where(w), where(first[0])))
                elif not any(r == got for r in slots_w.values()):
                    report(lst, j, o, slot, "writer", "reads %d bytes of %s; its producer %s wrote %s" %
                           (sum(b - a for a, b in got), owners.label(k), where(w),
                            " / ".join("%d bytes through %s" % (sum(b - a for a, b in r), sl) for sl, r in slots_w.items())))

    # ---- the consumer of the step: reads the gradients, the output and dx on stream 0 after the last op
    end_clock = clock[0]
    for name in ("flat_grad", "out", "dx"):
        k = next((k for k, r in enumerate(owners.ranges) if r[2] == name), None)
        if k is None:
            continue
        for seg in maps[k].segs:
            if seg.writer not in (None, _START) and not hb(seg.writer, end_clock):
                lst, j, o, _, _ = ops_seq[seg.writer]
                slot = next((sl for (op_, sl, k_), r in writes.items() if op_ == seg.writer and k_ == k
                             and any(a <= seg.a < b for a, b in r)), "")
                report(lst, j, o, slot, "order", "its write of %s is not joined into stream 0 by the end of the lists" % name)
    for (start, n), hits in cover_hits.items():
        label, want = cover[(start, n)]
        if hits != want:
            acc[("params", -1, label)] = [["cover"], ["%d launches target the gradient of %s; it has %d applications" % (hits, label, want)], ""]
    return [Finding(lst, j, e[2], slot, "+".join(e[0]), "; ".join(e[1])) for (lst, j, slot), e in acc.items()]


def event_counter():
    """A stand-in for Engine.new_event (set it on the instance): a plan with a side stream then builds without a device -- the
    handles are only ever stored in ops."""
    state = {"n": 0}

    def new_event():
        state["n"] += 1
        return 0x1000 + state["n"]
    return new_event
