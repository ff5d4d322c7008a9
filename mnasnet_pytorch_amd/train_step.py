"""The training step of the reference (``src/train.py:423-440``) on MI355X, single- and multi-GPU.

    input = input.float().to(device); out = model(input); loss = criterion(out, target)
    optimizer.zero_grad(); loss.backward(); optimizer.step()

Reference parallelism: one ``torch.nn.DataParallel`` call (train.py:202): single process, batch scattered
along dim 0, per-replica (UNSYNCED) BatchNorm statistics, gradients reduce-added, replica-0 buffers win.
Here: one process per GPU (``torch.distributed`` backend "nccl" = RCCL over xGMI), the same per-rank BatchNorm
semantics, and ONE flat fp32 gradient buffer laid out in the order gradients become final during backward
    [ classifier head | features.7 | features.6 | ... | features.0 ]
so the all-reduce runs as two contiguous buckets: bucket 0 (head + late stages: >80 % of the bytes) is
launched from the engine's stage-done callback while the early, activation-heavy stages are still running
backward; bucket 1 at the end.  The payload is ~8.9 MB: latency-bound on xGMI, so few large buckets, not many
small ones.  The optimizer is one fused Adam launch over the flat parameter buffer
(``mnas_adam_step``; torch.optim.Adam semantics, train.py:219-221), with the 1/world_size averaging folded in.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from typing import List, NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib as L


class FlatBuckets:
    """Contiguous [start, end) element ranges of a flat gradient buffer, all-reduced asynchronously.
    Pure host logic + torch.distributed: exercised on CPU/gloo by tests/test_ddp_gloo.py."""

    def __init__(self, flat: torch.Tensor, bounds: List[int], group=None):
        assert bounds[0] == 0 and bounds[-1] == flat.numel() and all(a <= b for a, b in zip(bounds, bounds[1:]))
        self.flat, self.bounds, self.group = flat, bounds, group
        self.handles = []

    @property
    def n(self):
        return len(self.bounds) - 1

    def launch(self, i: int):
        import torch.distributed as dist
        a, b = self.bounds[i], self.bounds[i + 1]
        if b > a:
            self.handles.append(dist.all_reduce(self.flat[a:b], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def wait(self):
        for h in self.handles:
            h.wait()
        self.handles = []


class BucketSchedule:
    """WHEN the two gradient buckets are all-reduced during backward (pure host logic; tests/test_ddp_gloo.py drives it
    with a stub engine on CPU/gloo).

    The flat gradient buffer is ``[head | engine stages, later stages first]``.  Bucket 0 = head + every stage >=
    ``early_bucket_stage`` (>80 % of the bytes: the late stages hold the wide weights) and is complete as soon as the backward
    of stage ``early_stage`` (= the smallest such stage present) has been enqueued -- the engine's stage-done callback fires
    right there, so the all-reduce runs under the backward of the early, activation-heavy stages.  Bucket 1 = the rest, launched
    at the end of backward.  ``join_stages`` = the stages after which the engine must join its weight-gradient side stream
    (bucket 0's gradients have to be complete on the stream the collective is ordered after)."""

    def __init__(self, flat_g: torch.Tensor, n_head: int, stage_ranges, early_bucket_stage: int, group=None):
        n = flat_g.numel()
        early = [s for s in stage_ranges if s >= early_bucket_stage]
        split = n_head + (max(stage_ranges[s][1] for s in early) if early else 0)
        self.buckets = FlatBuckets(flat_g, [0, split, n], group)
        self._n_head, self._stage_ranges, self._bounds = n_head, {s: tuple(r) for s, r in stage_ranges.items()}, [0, split, n]
        self.early_stage = min(early) if early else None
        self.join_stages = {self.early_stage} if self.early_stage is not None else set()
        self.launched0 = False
        self.log = []                     # ("stage", s) / ("launch", bucket): the order things happened in (tests)

    def begin_step(self, first_trainable_stage: int = 0):
        """first_trainable_stage: the stage the engine's backward ends in this step (a frozen stage prefix, Engine.first_trainable_step).
        The stages wholly in front of it have no gradient and are left out of the all-reduce: the flat layout is later stages
        first, so the trainable stages are a leading range and both buckets are clipped to it (an empty bucket launches nothing).
        Every rank must pass the same value: the collectives pair up by size."""
        self.launched0 = False
        self.log = []
        live = [s for s in self._stage_ranges if s >= first_trainable_stage]
        end = self._n_head + (max(self._stage_ranges[s][1] for s in live) if live else 0)
        self.buckets.bounds = [min(b, end) for b in self._bounds]

    def on_stage_done(self, stage: int):
        """engine callback: the backward of features.<stage> (and everything after it) has been enqueued"""
        self.log.append(("stage", stage))
        if not self.launched0 and self.early_stage is not None and stage <= self.early_stage:
            self.buckets.launch(0)
            self.launched0 = True
            self.log.append(("launch", 0))

    def finish(self):
        """end of backward: whatever has not been launched yet, then wait for both"""
        if not self.launched0:
            self.buckets.launch(0)
            self.launched0 = True
            self.log.append(("launch", 0))
        self.buckets.launch(1)
        self.log.append(("launch", 1))
        self.buckets.wait()


class GradStats(NamedTuple):
    """FlatAdam.grad_stats() / Trainer.grad_stats(): the MnasGradStats block (include/mnas.h) on the host"""
    last_norm: float
    last_coef: float
    steps: int
    clipped_steps: int
    skipped_steps: int


class OptTables(NamedTuple):
    """build_opt_tables(): the two tables of the ``mnas_*_step_seg`` calls (include/mnas.h) as host tuples"""
    segs: list        # (begin, n, group, tile0, ntiles, parameter index), one per trainable non-empty parameter tensor
    tiles: list       # (begin, n, segment index): at most `tile` consecutive elements of one segment


def build_opt_tables(ranges, requires_grad, group_index, tile=L.OPT_TILE) -> OptTables:
    """Pure host logic (tests/test_param_groups_cpu.py drives it without a device).  ``ranges``: the [begin, end) element range of
    every parameter tensor inside the flat buffers, in address order; ``requires_grad`` and ``group_index`` per tensor.  A frozen (or
    empty) tensor gets no segment, so nothing of it is read or written; a segment's tiles are consecutive, in element order, and
    never cross into the next tensor."""
    segs, tiles = [], []
    for i, ((a, b), rg, gi) in enumerate(zip(ranges, requires_grad, group_index)):
        if not rg or a == b:
            continue
        n, t0 = b - a, len(tiles)
        nt = -(-n // tile)
        for k in range(nt):
            tiles.append((a + k * tile, min(tile, n - k * tile), len(segs)))
        segs.append((a, n, int(gi), t0, nt, i))
    return OptTables(segs, tiles)


class FlatAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (train.py:219-221) over ONE flat fp32 buffer: a single fused launch (``mnas_adam_step``) instead
    of ~110 per-tensor updates.  It is a real ``torch.optim.Optimizer``:

    * ``param_groups[0]['lr']`` (and betas / eps / weight_decay) are read at every step, so the schedulers of the
      reference (MultiStepLR, ExponentialLR, ReduceLROnPlateau, CyclicLR.batch_step: train.py:284-337) and the
      ``optimizer.state_dict()['param_groups'][0]['lr']`` read-back (train.py:450) work unchanged;
    * ``state_dict()`` / ``load_state_dict()`` carry the moments and the step count (train.py:382 checkpoints them);
    * parameters with ``requires_grad == False`` (``FineTuneModelPool.freeze()``, classifiers.py:95-99) are left
      untouched: the update runs over the contiguous runs of trainable elements only, so weight decay cannot move a
      frozen weight.

    Three optional pieces of the step run on the same buffers without a host read (include/mnas.h).  They
    are plain attributes read at every step, like ``lr``, so a caller can schedule them (an EMA warm-up, say):

    * ``clip_grad_norm`` (None = off, else > 0): the gradient the update consumes -- ``flat_g * grad_scale`` over the trainable runs
      -- is scaled by ``min(1, clip_grad_norm / (norm + 1e-6))``, ``torch.nn.utils.clip_grad_norm_``'s arithmetic;
    * ``skip_nonfinite``: a step whose gradient norm is NaN / Inf changes neither the parameters nor the moments nor the EMA;
    * ``ema_decay`` (None = off, else in [0, 1)): ``flat_ema = d * flat_ema + (1 - d) * flat_p`` behind the update, in the same
      launch.  ``flat_ema`` is a copy of ``flat_p`` taken when the EMA is first enabled (:meth:`reset_ema` takes it again, e.g.
      after loading a checkpoint into the model).  Frozen parameters are outside the norm and the EMA update.

    With all three off ``step()`` issues exactly the plain launches.  Otherwise: one ``mnas_grad_sqnorm`` launch per trainable run
    (none when only the EMA is on), then one ``*_step_ex`` launch per run; :meth:`grad_stats` reads the device counters.

    Deviation on skipped steps: the skip is decided on the device, so the host ``step_count`` advances on a skipped step too
    (rolling it back would take the host read this path exists to avoid).  After a skip, Adam's bias correction and the native
    head's dropout seeds are therefore one step ahead of a torch run that skipped the same step, and SGD with ``dampening != 0``
    differs from it when step 1 is the skipped one (torch would seed the momentum buffer with the next gradient, undamped).

    Parameter groups, decoupled decay, trust ratios (include/mnas.h: ``mnas_*_step_seg``).  ``params`` may be
    a torch-style list of group dicts ``{"params": [...], "lr": ..., "weight_decay": ..., "decoupled": bool, "trust": bool}`` (what
    a group leaves out comes from the constructor); the union of the groups' parameters, ordered by address, must tile ``flat_p``
    exactly.  ``param_groups`` stays a real torch list read at every step, so a scheduler scales every group.  Per group: ``lr``,
    ``weight_decay``, ``decoupled`` (``p *= 1 - lr * weight_decay`` ahead of an update that sees the undecayed gradient: for Adam
    ``torch.optim.AdamW``; the constructor's ``decoupled_weight_decay`` is the default) and ``trust``.  The other hyper-parameters
    (betas, eps, alpha, momentum, ...) are per optimizer and read from ``param_groups[0]``.  ``trust_ratio="lamb"`` (FlatAdam) /
    ``"lars"`` (FlatSGD) scales every tensor's update by a layer-wise ratio of deterministic fp64 norms; a group with
    ``trust=False`` (BatchNorm parameters, biases) keeps ratio 1, and a group cannot be decoupled and take a trust ratio (LAMB and
    LARS carry the decay inside the ratio'd update).  :meth:`trust_ratios` reads the last step's ratios.

    Routing: ONE group with none of these options takes exactly the launches described above (same launches, same bits).
    Anything else is one ``mnas_*_step_seg`` call per step that updates the whole buffer in one launch -- two short launches more
    for the norms of a trust-ratio step -- from device tables (one segment per trainable tensor) that are rebuilt only when the
    ``requires_grad`` pattern or the groups' membership changes.  The global gradient norm is ``mnas_grad_sqnorm`` per trainable
    run, unchanged.
    """
    _trust_name = "lamb"                  # the trust ratio this optimizer supports (FlatRMSprop: none, FlatSGD: "lars")

    def __init__(self, params, flat_p, flat_g, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                 clip_grad_norm=None, skip_nonfinite=False, ema_decay=None, decoupled_weight_decay=False, trust_ratio=None,
                 trust_coef=1e-3, trust_eps=1e-8):
        params = list(params)
        grouped = bool(params) and isinstance(params[0], dict)
        if grouped:
            if len(params) > L.OPT_MAX_GROUPS:
                raise ValueError("at most %d parameter groups (MNAS_OPT_MAX_GROUPS), got %d" % (L.OPT_MAX_GROUPS, len(params)))
            groups = [dict(g, params=list(g["params"])) for g in params]
            every = [p for g in groups for p in g["params"]]
            if len({id(p) for p in every}) != len(every):
                raise ValueError("a parameter appears in more than one parameter group")
            every.sort(key=lambda p: p.data_ptr())
        else:
            groups, every = None, params
        n = sum(p.numel() for p in every)
        if flat_p.numel() != n or flat_g.numel() != n:
            raise ValueError("flat buffers must hold exactly the parameters handed to FlatAdam")
        off = 0
        self._ranges = []                 # element range of every parameter inside the flat buffers
        for p in every:
            if p.data_ptr() != flat_p.data_ptr() + 4 * off:
                raise ValueError("parameters must be views of flat_p in order" if not grouped else
                                 "the groups' parameters, ordered by address, must tile flat_p exactly")
            self._ranges.append((off, off + p.numel()))
            off += p.numel()
        self._all_params = every          # every parameter, in ADDRESS order: what _ranges is indexed by (a group dict may list
                                          # its parameters in any order, so param_groups[k]['params'] is not)
        self.trust_ratio, self.trust_coef, self.trust_eps = trust_ratio, trust_coef, trust_eps
        self._check_trust()
        super().__init__(groups if grouped else params,
                         dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=bool(decoupled_weight_decay),
                              trust=trust_ratio is not None))
        self._check_groups()
        self._seg_key, self._seg = None, None     # the device tables of the _seg path and what they were built for
        self.flat_p, self.flat_g = flat_p, flat_g
        self.flat_m = torch.zeros_like(flat_p)
        self.flat_v = torch.zeros_like(flat_p)
        self.step_count = 0
        self.seg_calls = 0                # mnas_*_step_seg calls issued so far (0 for ever on the one-group path)
        self.grad_scale = grad_scale      # 1/world_size: the all-reduce sums, Adam sees the mean (DataParallel semantics)
        self._lib = L.load()
        self._runs_key, self._runs = None, []
        self.clip_grad_norm, self.skip_nonfinite, self.ema_decay = clip_grad_norm, bool(skip_nonfinite), ema_decay
        self._check_extras()
        self.flat_ema = None              # the EMA shadow of flat_p (allocated when the EMA is first enabled)
        self._partial = None              # MNAS_GRADNORM_MAX_PARTS doubles: the norm launches' partial sums
        self._stats = None                # one MnasGradStats block, as 4 int64 (the two floats share the first)
        if ema_decay is not None:
            self.reset_ema()

    # ---- gradient clipping / non-finite skip / EMA ------------------------------------------------------------------------
    def _check_extras(self):
        """the three attributes, before anything is launched (the constructor and every step with one of them on call it)"""
        c, d = self.clip_grad_norm, self.ema_decay
        if c is not None and not float(c) > 0.0:
            raise ValueError("clip_grad_norm must be > 0 (None: no clipping), got %r" % (c,))
        if d is not None and not 0.0 <= float(d) < 1.0:
            raise ValueError("ema_decay must be in [0, 1) (None: no EMA), got %r" % (d,))

    def reset_ema(self):
        """flat_ema = a copy of the current parameters"""
        if self.flat_ema is None:
            self.flat_ema = self.flat_p.detach().clone()
        else:
            self.flat_ema.copy_(self.flat_p)

    def _stats_block(self):
        if self._stats is None:
            assert ctypes.sizeof(L.MnasGradStats) == 32
            self._stats = torch.zeros(4, dtype=torch.int64, device=self.flat_p.device)
        return self._stats

    @property
    def last_grad_norm(self):
        """device tensor view (one fp32 element) of MnasGradStats.last_norm: no sync"""
        return self._stats_block().view(torch.float32)[0:1]

    def grad_stats(self):
        """ONE device-to-host copy of the MnasGradStats block (waits for what was enqueued before it)."""
        host = self._stats_block().cpu()
        raw = L.MnasGradStats()
        ctypes.memmove(ctypes.byref(raw), host.data_ptr(), ctypes.sizeof(raw))
        return GradStats(float(raw.last_norm), float(raw.last_coef), int(raw.steps), int(raw.clipped_steps), int(raw.skipped_steps))

    # ---- parameter groups / decoupled decay / trust ratios ------------------------------------------------------------------
    def _check_trust(self):
        """the trust-ratio attributes, before anything is launched"""
        t = self.trust_ratio
        if t not in (None, "lamb", "lars"):
            raise ValueError("trust_ratio must be None, 'lamb' or 'lars', got %r" % (t,))
        if t is not None and t != self._trust_name:
            raise ValueError("trust_ratio=%r is not available on %s (LAMB is Adam's, LARS is SGD's, RMSprop has none)"
                             % (t, type(self).__name__))
        if t is not None:
            c, e = float(self.trust_coef), float(self.trust_eps)
            if c != c or e != e or e < 0.0:
                raise ValueError("trust_coef must be a number and trust_eps >= 0, got %r, %r" % (self.trust_coef, self.trust_eps))

    def _check_groups(self):
        """every group's flags and scalars (the constructor and every grouped step call it: the groups are plain dicts)"""
        if len(self.param_groups) > L.OPT_MAX_GROUPS:
            raise ValueError("at most %d parameter groups (MNAS_OPT_MAX_GROUPS), got %d" % (L.OPT_MAX_GROUPS, len(self.param_groups)))
        for k, g in enumerate(self.param_groups):
            if self.trust_ratio is not None and g["decoupled"] and g["trust"]:
                raise ValueError("parameter group %d: decoupled weight decay and a trust ratio exclude each other (LAMB / LARS carry "
                                 "the decay inside the ratio'd update)" % k)
            if float(g["lr"]) != float(g["lr"]) or float(g["weight_decay"]) != float(g["weight_decay"]):
                raise ValueError("parameter group %d: lr / weight_decay is NaN" % k)

    def _grouped(self):
        """False: one group with none of the new options -- today's launches"""
        return len(self.param_groups) > 1 or self.trust_ratio is not None or bool(self.param_groups[0]["decoupled"])

    def _seg_tables(self):
        """the device tables of the _seg call, rebuilt when the requires_grad pattern or the groups' membership changes"""
        member = {}
        for k, g in enumerate(self.param_groups):
            for p in g["params"]:
                if id(p) in member:
                    raise ValueError("a parameter appears in more than one parameter group")
                member[id(p)] = k
        try:
            gidx = tuple(member[id(p)] for p in self._all_params)
        except KeyError:
            raise ValueError("the parameter groups no longer hold every parameter of the flat buffer") from None
        if len(member) != len(self._all_params):
            raise ValueError("the parameter groups hold a parameter that is not in the flat buffer")
        key = (tuple(p.requires_grad for p in self._all_params), gidx, self.trust_ratio is not None)
        if key != self._seg_key:
            tb = build_opt_tables(self._ranges, key[0], gidx)
            if len(tb.segs) > L.OPT_MAX_SEGS:
                raise ValueError("%d trainable parameter tensors: more than MNAS_OPT_MAX_SEGS = %d" % (len(tb.segs), L.OPT_MAX_SEGS))
            dev = self.flat_p.device

            def upload(cls, rows):
                arr = (cls * max(1, len(rows)))(*[cls(*r) for r in rows])
                return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)

            seg = {"tables": tb, "segs": upload(L.MnasOptSeg, [s[:5] + (0,) for s in tb.segs]), "tiles": upload(L.MnasOptTile, tb.tiles),
                   "partial": None, "ratio": None, "groups": (L.MnasOptGroup * L.OPT_MAX_GROUPS)()}
            if self.trust_ratio is not None:
                seg["partial"] = torch.zeros(2 * max(1, len(tb.tiles)), dtype=torch.float64, device=dev)
                seg["ratio"] = torch.ones(max(1, len(tb.segs)), dtype=torch.float32, device=dev)
            self._seg_key, self._seg = key, seg
        return self._seg

    @property
    def last_trust_ratios(self):
        """device tensor: the last trust-ratio step's ratio of every segment (trainable tensor, address order, as that step's
        tables had them); None without ``trust_ratio`` or before the first such step.  A plain read: no sync, and the tables are
        not rebuilt here, so a ``requires_grad`` or membership change shows from the next step on."""
        seg = self._seg
        if self.trust_ratio is None or seg is None or seg["ratio"] is None or not self.seg_calls:
            return None
        return seg["ratio"][:len(seg["tables"].segs)]

    def trust_ratios(self):
        """{parameter index (address order, as in the flat buffer): ratio of the last step} from ONE host read; frozen tensors
        are absent, a ``trust=False`` group's tensors read 1.0.  {} without ``trust_ratio`` or before the first step.  The
        indices and the frozen set are the LAST STEP's (see :attr:`last_trust_ratios`)."""
        dev = self.last_trust_ratios
        if dev is None:
            return {}
        return {s[5]: r for s, r in zip(self._seg["tables"].segs, dev.cpu().tolist())}

    def _step_seg(self, runs):
        """one mnas_*_step_seg call: every group, the whole buffer"""
        self._check_extras()
        self._check_trust()
        self._check_groups()
        seg = self._seg_tables()
        tb = seg["tables"]
        if not tb.segs:
            return
        ex = None
        if self.clip_grad_norm is not None or self.skip_nonfinite or self.ema_decay is not None:
            if self.ema_decay is not None and self.flat_ema is None:
                self.reset_ema()
            ex = self._extra(self._norm_launches(runs))
            ex.ema = self.flat_ema.data_ptr() if self.ema_decay is not None else None
            ex.update_stats = 1
        trust = self.trust_ratio is not None
        for k, g in enumerate(self.param_groups):
            seg["groups"][k] = L.MnasOptGroup(float(g["lr"]), float(g["weight_decay"]), 1 if g["decoupled"] else 0,
                                              1 if trust and g["trust"] else 0)
        segs = L.MnasOptSegs(segs=seg["segs"].data_ptr(), tiles=seg["tiles"].data_ptr(), groups=seg["groups"], nsegs=len(tb.segs),
                             ntiles=len(tb.tiles), ngroups=len(self.param_groups),
                             trust_kind={None: L.TRUST_NONE, "lamb": L.TRUST_LAMB, "lars": L.TRUST_LARS}[self.trust_ratio],
                             tile_partial=L.ptr(seg["partial"]), ratio=L.ptr(seg["ratio"]),
                             trust_coef=float(self.trust_coef), trust_eps=float(self.trust_eps))
        self.seg_calls += 1
        self._launch_seg(self.param_groups[0], segs, ex)

    def _launch_seg(self, g, segs, ex):
        L.check(self._lib.mnas_adam_step_seg(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_m.data_ptr(),
                                             self.flat_v.data_ptr(), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                             self.step_count, float(self.grad_scale), ctypes.byref(segs),
                                             ctypes.byref(ex) if ex is not None else None, L.cur_stream()), "adam_step_seg")

    def _norm_launches(self, runs):
        """mnas_grad_sqnorm per trainable run into consecutive slots of one table (clipping or the skip on) -> used slots"""
        stream = L.cur_stream()
        nparts = 0
        if self.clip_grad_norm is not None or self.skip_nonfinite:
            if self._partial is None:
                self._partial = torch.zeros(L.GRADNORM_MAX_PARTS, dtype=torch.float64, device=self.flat_p.device)
            got = ctypes.c_int(0)
            for a, b in runs:
                L.check(self._lib.mnas_grad_sqnorm(self.flat_g.data_ptr() + 4 * a, b - a, float(self.grad_scale),
                                                   self._partial.data_ptr(), nparts, ctypes.byref(got), stream), "grad_sqnorm")
                nparts += got.value
        return nparts

    def _extra(self, nparts):
        clip = self.clip_grad_norm
        return L.MnasOptExtra(partial=L.ptr(self._partial) if nparts else None, nparts=nparts,
                              max_norm=float(clip) if clip is not None and math.isfinite(float(clip)) else 0.0,
                              skip_nonfinite=1 if self.skip_nonfinite else 0, ema=None,
                              ema_decay=float(self.ema_decay) if self.ema_decay is not None else 0.0,
                              stats=self._stats_block().data_ptr(), update_stats=0)

    def _step_extras(self, g, runs):
        """the step with clipping, the skip or the EMA on: norm launches into consecutive slots of one table, then the _ex launches"""
        self._check_extras()
        if self.ema_decay is not None and self.flat_ema is None:
            self.reset_ema()
        ex = self._extra(self._norm_launches(runs))
        for k, (a, b) in enumerate(runs):
            ex.ema = self.flat_ema.data_ptr() + 4 * a if self.ema_decay is not None else None
            ex.update_stats = 1 if k == 0 else 0
            self._launch(a, b, g, ex)

    def _trainable_runs(self):
        key = tuple(p.requires_grad for p in self._all_params)      # address order, like _ranges
        if key != self._runs_key:
            runs = []
            for (a, b), rg in zip(self._ranges, key):
                if not rg or a == b:
                    continue
                if runs and runs[-1][1] == a:
                    runs[-1][1] = b
                else:
                    runs.append([a, b])
            self._runs_key, self._runs = key, runs
        return self._runs

    def zero_grad(self, set_to_none: bool = False):
        """The gradients are views of the flat buffer: zero it in one launch (never set to None)."""
        self.flat_g.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        self.step_count += 1
        runs = self._trainable_runs()
        if self._grouped():
            self._step_seg(runs)
            return loss
        if self.clip_grad_norm is not None or self.skip_nonfinite or self.ema_decay is not None:
            self._step_extras(g, runs)
            return loss
        for a, b in runs:
            self._launch(a, b, g)
        return loss

    def _launch(self, a, b, g, ex=None):
        """the update of flat elements [a, b); ex: a MnasOptExtra -> the _ex entry point"""
        args = (self.flat_p.data_ptr() + 4 * a, self.flat_g.data_ptr() + 4 * a,
                self.flat_m.data_ptr() + 4 * a, self.flat_v.data_ptr() + 4 * a, b - a,
                float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                float(g["weight_decay"]), self.step_count, float(self.grad_scale))
        if ex is None:
            L.check(self._lib.mnas_adam_step(*args, L.cur_stream()), "adam_step")
        else:
            L.check(self._lib.mnas_adam_step_ex(*args, ctypes.byref(ex), L.cur_stream()), "adam_step_ex")

    def state_dict(self):
        state = {"step": self.step_count, "exp_avg": self.flat_m.clone(), "exp_avg_sq": self.flat_v.clone()}
        if self.ema_decay is not None:
            if self.flat_ema is None:
                self.reset_ema()
            state["ema"] = self.flat_ema.clone()
        groups, k = [], 0                 # torch's layout: every group, its parameters numbered consecutively in group order
        for g in self.param_groups:
            groups.append({key: v for key, v in g.items() if key != "params"} | {"params": list(range(k, k + len(g["params"])))})
            k += len(g["params"])
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        st = sd["state"]
        if st["exp_avg"].numel() != self.flat_m.numel():
            raise ValueError("optimizer state has %d elements, this model %d" % (st["exp_avg"].numel(), self.flat_m.numel()))
        self.step_count = int(st["step"])
        self.flat_m.copy_(st["exp_avg"].to(self.flat_m.device))
        self.flat_v.copy_(st["exp_avg_sq"].to(self.flat_v.device))
        if "ema" in st:
            if st["ema"].numel() != self.flat_p.numel():
                raise ValueError("EMA state has %d elements, this model %d" % (st["ema"].numel(), self.flat_p.numel()))
            if self.flat_ema is None:
                self.flat_ema = torch.empty_like(self.flat_p)
            self.flat_ema.copy_(st["ema"].to(self.flat_ema.device))
        elif self.ema_decay is not None:
            self.reset_ema()              # a checkpoint written with the EMA off: the shadow restarts from the current parameters
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("loaded state dict has %d parameter groups, this optimizer %d" % (len(sd["param_groups"]), len(self.param_groups)))
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            if len(saved["params"]) != len(g["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            for k, v in saved.items():      # (a checkpoint from before the groups has no 'decoupled' / 'trust': they stay as constructed)
                if k != "params":
                    g[k] = v


class FlatRMSprop(FlatAdam):
    """``torch.optim.RMSprop`` (train.py:222-224: ``--optimizer rmsprop``; alpha 0.99, eps 1e-8, centered = False) over the flat
    buffers: one fused launch (``mnas_rmsprop_step``).  Same Optimizer contract as :class:`FlatAdam`, parameter groups and
    decoupled decay included; no trust ratio."""
    _trust_name = None

    def __init__(self, params, flat_p, flat_g, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False,
                 grad_scale=1.0, **extras):
        if centered:
            raise NotImplementedError("centered RMSprop is not fused (the reference never asks for it: train.py:222-224)")
        super().__init__(params, flat_p, flat_g, lr=lr, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, **extras)
        self.defaults.pop("betas", None)
        self.defaults.update(alpha=alpha, momentum=momentum, centered=False)
        for g in self.param_groups:
            g.pop("betas", None)
            for k in ("alpha", "momentum", "centered"):
                g.setdefault(k, self.defaults[k])
        # flat_m = momentum buffer, flat_v = square average (same checkpoint layout as FlatAdam: exp_avg / exp_avg_sq)

    def _launch(self, a, b, g, ex=None):
        args = (self.flat_p.data_ptr() + 4 * a, self.flat_g.data_ptr() + 4 * a,
                self.flat_v.data_ptr() + 4 * a, self.flat_m.data_ptr() + 4 * a, b - a, float(g["lr"]),
                float(g["alpha"]), float(g["eps"]), float(g["weight_decay"]), float(g["momentum"]), float(self.grad_scale))
        if ex is None:
            L.check(self._lib.mnas_rmsprop_step(*args, L.cur_stream()), "rmsprop_step")
        else:
            L.check(self._lib.mnas_rmsprop_step_ex(*args, ctypes.byref(ex), L.cur_stream()), "rmsprop_step_ex")

    def _launch_seg(self, g, segs, ex):
        L.check(self._lib.mnas_rmsprop_step_seg(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_v.data_ptr(),
                                                self.flat_m.data_ptr(), float(g["alpha"]), float(g["eps"]), float(g["momentum"]),
                                                float(self.grad_scale), ctypes.byref(segs),
                                                ctypes.byref(ex) if ex is not None else None, L.cur_stream()), "rmsprop_step_seg")


class FlatSGD(FlatAdam):
    """``torch.optim.SGD`` (train.py:226-228: ``--optimizer sgd``; momentum 0 by default) over the flat buffers
    (``mnas_sgd_step``).  ``flat_m`` is the momentum buffer (initialised with the first gradient, as torch does).  Parameter
    groups and decoupled decay as :class:`FlatAdam`; ``trust_ratio="lars"``."""
    _trust_name = "lars"

    def __init__(self, params, flat_p, flat_g, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0,
                 **extras):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, flat_p, flat_g, lr=lr, weight_decay=weight_decay, grad_scale=grad_scale, **extras)
        for k in ("betas", "eps"):
            self.defaults.pop(k, None)
        self.defaults.update(momentum=momentum, dampening=dampening, nesterov=nesterov)
        for g in self.param_groups:
            g.pop("betas", None)
            g.pop("eps", None)
            for k in ("momentum", "dampening", "nesterov"):
                g.setdefault(k, self.defaults[k])

    def _launch(self, a, b, g, ex=None):
        args = (self.flat_p.data_ptr() + 4 * a, self.flat_g.data_ptr() + 4 * a,
                self.flat_m.data_ptr() + 4 * a, b - a, float(g["lr"]), float(g["momentum"]),
                float(g["dampening"]), float(g["weight_decay"]), 1 if g["nesterov"] else 0, self.step_count,
                float(self.grad_scale))
        if ex is None:
            L.check(self._lib.mnas_sgd_step(*args, L.cur_stream()), "sgd_step")
        else:
            L.check(self._lib.mnas_sgd_step_ex(*args, ctypes.byref(ex), L.cur_stream()), "sgd_step_ex")

    def _launch_seg(self, g, segs, ex):
        L.check(self._lib.mnas_sgd_step_seg(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_m.data_ptr(),
                                            float(g["momentum"]), float(g["dampening"]), 1 if g["nesterov"] else 0, self.step_count,
                                            float(self.grad_scale), ctypes.byref(segs),
                                            ctypes.byref(ex) if ex is not None else None, L.cur_stream()), "sgd_step_seg")


def norm_bias_groups(model: nn.Module, weight_decay: float):
    """Two parameter groups: tensors with ``ndim <= 1`` (BatchNorm weights and biases, conv / linear biases) get no weight decay
    and no trust ratio, everything else ``weight_decay`` -- torchvision's ``--norm-weight-decay 0`` and the published MnasNet
    setting.  For ``Trainer(param_groups=...)`` (as a callable: ``lambda m: norm_bias_groups(m, 1e-5)``) or the optimizers."""
    decay, no_decay = [], []
    for p in model.parameters():
        (no_decay if p.ndim <= 1 else decay).append(p)
    return [{"params": decay, "weight_decay": weight_decay}, {"params": no_decay, "weight_decay": 0.0, "trust": False}]


def stage_lr_groups(model: nn.Module, lr: float, decay: float, groups=None):
    """Layer-wise learning-rate decay for fine-tuning: the head trains at ``lr``, ``model.features[k]`` at
    ``lr * decay ** (len(model.features) - 1 - k)`` (the eight MnasNet stages: ``decay ** (7 - k)``).  ``groups``: a list of group
    dicts to split by stage, their other keys kept (``stage_lr_groups(m, lr, d, norm_bias_groups(m, wd))``: at most 18 groups);
    None: all of the model's parameters."""
    feats = model.features
    stage_of = {id(p): k for k, child in enumerate(feats) for p in child.parameters()}
    out = []
    for g in (groups if groups is not None else [{"params": list(model.parameters())}]):
        by_stage = {}
        for p in g["params"]:
            by_stage.setdefault(stage_of.get(id(p), len(feats)), []).append(p)
        for k in sorted(by_stage, reverse=True):
            out.append({**g, "params": by_stage[k], "lr": lr * decay ** max(0, len(feats) - 1 - k)})
    return out


class Trainer:
    """Owns flat parameter / gradient / Adam-moment buffers for ``model`` (a FineTuneModelPool or anything with
    a ``features`` engine module plus ordinary PyTorch head parameters) and runs train.py's step.
    ``trainer.optimizer`` is a :class:`FlatAdam` (a ``torch.optim.Optimizer``): hand it to the reference's schedulers and
    checkpoint it with ``optimizer.state_dict()`` exactly as train.py does.  ``clip_grad_norm=``, ``skip_nonfinite=`` and
    ``ema_decay=`` go to the optimizer (see :class:`FlatAdam`); in a distributed trainer the norm is taken after the all-reduce with
    ``grad_scale = 1/world``, i.e. over the mean gradient, and is bit-identical on every rank.

    ``param_groups=`` (a list of torch-style group dicts, or a callable ``model -> list``, e.g. :func:`norm_bias_groups` and
    :func:`stage_lr_groups`; parameters no group names join a default group), ``decoupled_weight_decay=`` (AdamW; also for RMSprop and
    SGD), ``trust_ratio=`` / ``trust_coef=`` go to the optimizer too.  ``optimizer="lamb"`` is Adam with the LAMB trust ratio,
    ``optimizer="lars"`` SGD with the LARS one; :meth:`trust_ratios` reads them by parameter name.  ``optimizer="adamw"`` has always
    been accepted as plain Adam (the name is matched by prefix) and still is: pass ``decoupled_weight_decay=True`` for AdamW.  Data
    parallel needs no further collective: the per-tensor norms are taken after the all-reduce, on buffers that are identical on
    every rank, by a summation that does not depend on the grid."""

    def __init__(self, model: nn.Module, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 criterion: Optional[nn.Module] = None, distributed: bool = False, process_group=None,
                 early_bucket_stage: int = 5, optimizer: str = "adam", meters=None, teacher: Optional[nn.Module] = None,
                 param_groups=None, decoupled_weight_decay: bool = False, trust_ratio: Optional[str] = None,
                 trust_coef: float = 1e-3, **optimizer_kwargs):
        self.model = model
        self.teacher = teacher           # knowledge distillation: step() runs it in eval mode and wraps the target (_teach)
        self.meters = meters             # metrics.DeviceMeters / MultiLabelMeters or None: train.py:447,453-468 on the device
        self.native_step = True          # see _native_head()
        self.last_logits = None
        self.criterion = criterion if criterion is not None else nn.CrossEntropyLoss()   # train.py:277
        self._check_meters(meters)
        self._check_teacher()
        self.lib = L.load()
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("Trainer needs the model on an MI355X device (no CPU path)")
        self.device = dev
        if self._distill():
            self.criterion.to(dev)       # its class-weight buffer: the kernel takes a raw device pointer
        feats = model.features if hasattr(model, "features") else model
        self.engine = feats._engine()
        eng_params = list(self.engine.params)
        eng_ids = {id(p) for p in eng_params}
        head = [p for p in model.parameters() if id(p) not in eng_ids]
        self.head_params = head
        n_head = sum(p.numel() for p in head)
        n_eng = self.engine.grad_numel
        n = n_head + n_eng
        self.flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        # ---- parameters become views of flat_p (same element order as the gradient layout)
        off = 0
        with torch.no_grad():
            for p in head:
                k = p.numel()
                self.flat_p[off:off + k].copy_(p.reshape(-1))
                p.data = self.flat_p[off:off + k].view(p.shape)
                p.grad = self.flat_g[off:off + k].view(p.shape)      # autograd accumulates in place
                off += k
            for ci in sorted(self.engine.param_owners, key=lambda c: -c.stage):
                for j, p in enumerate(ci.params):
                    o, k = ci.gslice[j]
                    self.flat_p[n_head + o:n_head + o + k].copy_(p.reshape(-1))
                    p.data = self.flat_p[n_head + o:n_head + o + k].view(p.shape)
        self.engine.bind_grad_buffer(self.flat_g[n_head:])
        self.engine.ensure_setup(dev)
        for p, v in zip(self.engine.params, self.engine.grad_views):
            p.grad = v                                                # "already ours" -> engine accumulates
        # flat order = head parameters, then the engine's (later stages first): FlatAdam checks the views line up
        # ---- data parallel
        self.distributed = distributed
        self.world = 1
        self.schedule: Optional[BucketSchedule] = None
        if distributed:
            import torch.distributed as dist
            self.world = dist.get_world_size(process_group)
            dist.broadcast(self.flat_p, src=0, group=process_group)     # identical replicas (DP semantics)
            self.schedule = BucketSchedule(self.flat_g, n_head, self.engine.stage_ranges, early_bucket_stage, process_group)
            self.engine.on_stage_done = self.schedule.on_stage_done
            # bucket 0 is all-reduced as soon as its last stage is done: its side-stream weight gradients must be in
            self.engine.join_stages = self.schedule.join_stages
            self.engine.reset_programs()
        # train.py:218-231: --optimizer adam | rmsprop | sgd, each constructed with lr only
        # "lamb" = Adam with the LAMB trust ratio, "lars" = SGD with the LARS one.  "adamw" has always been taken as plain Adam by
        # the prefix match below and still is: decoupled decay is asked for with decoupled_weight_decay=True.
        if optimizer == "lamb":
            optimizer, trust_ratio = "adam", "lamb"
        elif optimizer == "lars":
            optimizer, trust_ratio = "sgd", "lars"
        params = self._resolve_groups(param_groups, head + eng_params)
        optimizer_kwargs = dict(optimizer_kwargs, decoupled_weight_decay=decoupled_weight_decay, trust_ratio=trust_ratio,
                                trust_coef=trust_coef)
        if optimizer.startswith("adam"):
            self.optimizer = FlatAdam(params, self.flat_p, self.flat_g, lr=lr, betas=betas, eps=eps,
                                      weight_decay=weight_decay, grad_scale=1.0 / self.world, **optimizer_kwargs)
        elif optimizer.startswith("rmsprop"):
            self.optimizer = FlatRMSprop(params, self.flat_p, self.flat_g, lr=lr, weight_decay=weight_decay,
                                         grad_scale=1.0 / self.world, **optimizer_kwargs)
        elif optimizer.startswith("sgd"):
            self.optimizer = FlatSGD(params, self.flat_p, self.flat_g, lr=lr, weight_decay=weight_decay,
                                     grad_scale=1.0 / self.world, **optimizer_kwargs)
        else:
            raise ValueError("Optimizer not supported")            # train.py:231

    def _resolve_groups(self, param_groups, every):
        """``param_groups`` (None, a list of group dicts, or a callable model -> such a list) -> what the optimizer is built from.
        Parameters that no group names join one further group that takes the constructor's defaults."""
        if param_groups is None:
            return every
        groups = param_groups(self.model) if callable(param_groups) else param_groups
        groups = [dict(g, params=list(g["params"])) for g in groups]
        known = {id(p) for p in every}
        named = set()
        for g in groups:
            for p in g["params"]:
                if id(p) not in known:
                    raise ValueError("a parameter group names a tensor that is not a parameter of the model")
                if id(p) in named:
                    raise ValueError("a parameter appears in more than one parameter group")
                named.add(id(p))
        groups = [g for g in groups if g["params"]]
        rest = [p for p in every if id(p) not in named]
        if rest:
            groups.append({"params": rest})
        return groups

    def trust_ratios(self):
        """{parameter name: the last step's trust ratio} (``optimizer="lamb"`` / ``"lars"``; ONE host read).  Frozen parameters
        are absent, a ``trust=False`` group's read 1.0."""
        names = {id(p): k for k, p in self.model.named_parameters()}
        every = self.optimizer._all_params
        return {names.get(id(every[i]), "param%d" % i): r for i, r in self.optimizer.trust_ratios().items()}

    # convenience mirrors of the optimizer's hyper-parameters / state
    @property
    def lr(self):
        """group 0's learning rate (with several parameter groups: set the others through ``optimizer.param_groups`` or a scheduler)"""
        return self.optimizer.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        self.optimizer.param_groups[0]["lr"] = v

    @property
    def step_count(self):
        return self.optimizer.step_count

    @property
    def flat_m(self):
        return self.optimizer.flat_m

    @property
    def flat_v(self):
        return self.optimizer.flat_v

    def state_dict(self):
        """{'optimizer': FlatAdam.state_dict()} -- what train.py:382 stores under 'optimizer'."""
        return {"optimizer": self.optimizer.state_dict()}

    def load_state_dict(self, sd):
        self.optimizer.load_state_dict(sd["optimizer"])

    # ---- gradient clipping / non-finite skip / weight EMA (FlatAdam; Trainer(clip_grad_norm=, skip_nonfinite=, ema_decay=)) ----
    def grad_stats(self) -> GradStats:
        """The optimizer's device counters -- last_norm, last_coef, steps, clipped_steps, skipped_steps -- in ONE host read, the
        only one of this feature."""
        return self.optimizer.grad_stats()

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """Device tensor view of the last step's gradient norm (no sync: for loggers that batch their reads)."""
        return self.optimizer.last_grad_norm

    @property
    def flat_ema(self):
        return self.optimizer.flat_ema

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the body on the EMA weights: the CONTENTS of flat_p and flat_ema are swapped on entry and swapped back on exit, also
        when the body raises.  The parameters are views of flat_p and the engine packs its weights from them inside every forward,
        so the model, the engine and ``state_dict()`` all see the averaged weights and nothing else needs to be told.  BatchNorm
        running statistics are shared, not averaged (they are moving averages already).  Do not step inside the body."""
        opt = self.optimizer
        if opt.ema_decay is None or opt.flat_ema is None:
            raise RuntimeError("ema_weights() needs the EMA on (Trainer(..., ema_decay=d) or optimizer.ema_decay = d)")
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    @torch.no_grad()
    def _swap_ema(self):
        p, e = self.flat_p, self.optimizer.flat_ema
        t = p.clone()
        p.copy_(e)
        e.copy_(t)

    def validate_ema(self, batches, meters=None, transform=None, max_batches=None, reduce=True):
        """:meth:`validate` under the EMA weights: the pass runs inside :meth:`ema_weights`.  (A method of its own and not an
        ``ema=`` keyword of ``validate``: that signature is pinned by tests/test_metrics_cpu.py.)"""
        with self.ema_weights():
            return self.validate(batches, meters, transform, max_batches, reduce)

    def ema_state_dict(self):
        """``model.state_dict()`` under the EMA weights, cloned: the checkpoint to evaluate from (it loads into the reference model
        like any other state dict of this model)."""
        with self.ema_weights():
            return {k: v.detach().clone() for k, v in self.model.state_dict().items()}

    def _multilabel(self):
        """the criterion is this package's MultiClassBCELoss itself: the reference's multi-label branch (train.py:274-279).  A
        subclass may override forward(), so it keeps the module path, as a subclass of nn.CrossEntropyLoss does"""
        from .losses import MultiClassBCELoss
        return type(self.criterion) is MultiClassBCELoss

    def _mlloss(self):
        """the criterion is this package's MultiLabelLoss itself (the multi-label branch's asymmetric focal loss, pos_weight,
        smoothing, mixed label rows); a subclass keeps the module path, as for the other criteria"""
        from .losses import MultiLabelLoss
        return type(self.criterion) is MultiLabelLoss

    def _mixce(self):
        """the criterion is this package's MixCrossEntropyLoss itself (label smoothing, mixed batches); a subclass keeps the module
        path, as for the other criteria"""
        from .losses import MixCrossEntropyLoss
        return type(self.criterion) is MixCrossEntropyLoss

    def _distill(self):
        """the criterion is this package's DistillCrossEntropyLoss itself (class weights, smoothing, mixed batches, a teacher's
        logits); a subclass keeps the module path, as for the other criteria"""
        from .losses import DistillCrossEntropyLoss
        return type(self.criterion) is DistillCrossEntropyLoss

    def _check_target(self, target):
        """a mixing.MixedTarget goes to a MixCrossEntropyLoss or a DistillCrossEntropyLoss (or a subclass of either) only, a
        losses.DistillTarget to a DistillCrossEntropyLoss (or a subclass) only, a mixing.MixedLabels to a MultiLabelLoss (or a
        subclass) only: refused before anything is launched"""
        from .losses import DistillCrossEntropyLoss, DistillTarget, MixCrossEntropyLoss, MultiLabelLoss
        from .mixing import MixedLabels, MixedTarget
        if isinstance(target, MixedLabels):
            if not isinstance(self.criterion, MultiLabelLoss):
                raise TypeError("a MixedLabels (a label matrix, partner rows and a weight per row) needs criterion=MultiLabelLoss(...); "
                                "%s takes no mixed label matrix" % type(self.criterion).__name__)
            return
        if isinstance(target, DistillTarget):
            if not isinstance(self.criterion, DistillCrossEntropyLoss):
                raise TypeError("a DistillTarget (labels and a teacher's logits) needs criterion=DistillCrossEntropyLoss(...); %s takes "
                                "no teacher logits" % type(self.criterion).__name__)
            return
        if isinstance(target, MixedTarget) and not isinstance(self.criterion, (MixCrossEntropyLoss, DistillCrossEntropyLoss)):
            raise TypeError("a MixedTarget (two labels and a weight per row) needs criterion=MixCrossEntropyLoss(...) or "
                            "DistillCrossEntropyLoss(...); %s takes no mixed batch" % type(self.criterion).__name__)

    def _check_teacher(self):
        """a teacher needs the criterion that takes its logits (the constructor and every step call it: both are plain attributes)"""
        from .losses import DistillCrossEntropyLoss
        if self.teacher is None:
            return
        if not isinstance(self.teacher, nn.Module):
            raise TypeError("teacher must be an nn.Module, got %s" % type(self.teacher).__name__)
        if not isinstance(self.criterion, DistillCrossEntropyLoss):
            raise TypeError("Trainer(teacher=...) needs criterion=DistillCrossEntropyLoss(...); %s takes no teacher logits"
                            % type(self.criterion).__name__)

    def _teach(self, x, target):
        """``teacher(x)`` in eval mode under ``torch.no_grad()`` -> a losses.DistillTarget around ``target``.  The teacher's
        train/eval flags are restored on the way out, also when its forward raises; nothing of the teacher is written (eval mode:
        its BatchNorm statistics stay, its engine runs the eval program).  A target that already is a DistillTarget (cached teacher
        logits) is taken as it is and the teacher is not run."""
        from .losses import DistillTarget
        from .mixing import MixedTarget
        if isinstance(target, DistillTarget):
            return target
        if not isinstance(target, (torch.Tensor, MixedTarget)) or target.device != x.device:
            raise RuntimeError("target must be a tensor on the input's device (%s)" % (x.device,))
        teacher = self.teacher
        modes = [(mod, mod.training) for mod in teacher.modules()]
        try:
            teacher.eval()
            with torch.no_grad():
                out = teacher(x)
        finally:
            for mod, flag in modes:
                mod.training = flag
        if (not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape[0] != x.shape[0] or out.dtype != torch.float32
                or out.device != x.device):
            raise ValueError("the teacher must return (N, C) fp32 logits on the batch's device (%s), got %s"
                             % (x.device, "%s %s on %s" % (out.dtype, tuple(out.shape), out.device) if isinstance(out, torch.Tensor)
                                else type(out).__name__))
        return DistillTarget(target, out)

    def _check_meters(self, meters):
        """the meters' kind against the criterion's, before anything is launched (the constructor, every forward_backward and
        validate call it: ``criterion`` and ``meters`` are plain attributes)"""
        from .losses import DistillCrossEntropyLoss, MixCrossEntropyLoss, MultiClassBCELoss, MultiLabelLoss
        from .metrics import MultiLabelMeters
        if meters is not None and isinstance(self.criterion, MultiLabelLoss) and not isinstance(meters, MultiLabelMeters):
            raise ValueError("a MultiLabelLoss step feeds MultiLabelMeters, not %s" % type(meters).__name__)
        if isinstance(meters, MultiLabelMeters) and isinstance(self.criterion, (nn.CrossEntropyLoss, MixCrossEntropyLoss,
                                                                               DistillCrossEntropyLoss)):
            raise ValueError("MultiLabelMeters count (N, C) multi-label targets; a cross-entropy criterion takes class indices "
                             "(use DeviceMeters)")
        if meters is not None and isinstance(self.criterion, MultiClassBCELoss) and not isinstance(meters, MultiLabelMeters):
            raise ValueError("a MultiClassBCELoss step feeds MultiLabelMeters, not %s" % type(meters).__name__)

    def _native_head(self):
        """The model's NativeHead when the whole step can bypass autograd: FineTuneModelPool-like model in training mode
        (fused pool, Dropout/Linear/ReLU classifier) and a plain mean-reduced nn.CrossEntropyLoss (train.py:277), this package's
        MultiClassBCELoss, its MixCrossEntropyLoss or its DistillCrossEntropyLoss.  The features may
        be entirely in eval mode under a training model (FineTuneModelPool.freeze_bn): forward_backward then runs the engine's
        frozen-statistics program; a subtree in mixed modes is refused by Engine._check_modes."""
        m = self.model
        head = self._native_eval_head()
        if head is None or not m.training:
            return None
        if any(not p.requires_grad for p in self.head_params):
            return None
        if self._frozen_prefix() is None:
            return None            # all features frozen (FineTuneModelPool.freeze()) or a pattern that is no stage prefix: module path
        return head

    def _frozen_prefix(self):
        """The engine step the native step's backward ends at: 0 with every engine parameter trainable, b when the frozen ones are
        exactly those of the steps in front of step b (FineTuneModelPool.freeze(upto=k)), 0 < b < len(steps).  None for anything
        else -- a frozen parameter behind the boundary, or nothing trainable at all: those keep the module path, which runs the
        truncated program too (engine._EngineFn)."""
        eng = self.engine
        b = eng.first_trainable_step()
        if b >= len(eng.steps):
            return None
        if any(not p.requires_grad for i in range(b, len(eng.steps)) for p in eng.step_params(i)):
            return None
        return b

    def _native_eval_head(self):
        """The part of _native_head() that does not concern training: what lets a validation batch run as engine forward (fused
        pool) -> head -> fused loss."""
        m, c = self.model, self.criterion
        if not self.native_step:
            return None
        if self._multilabel() or self._mlloss() or self._mixce() or self._distill():
            pass                   # losses.MultiClassBCELoss / MultiLabelLoss / MixCrossEntropyLoss / DistillCrossEntropyLoss: every
                                   # setting is covered (head.NativeHead.bce, .mlabel, .cross_entropy_soft, .cross_entropy_kd)
        elif type(c) is not nn.CrossEntropyLoss:
            return None
        elif c.weight is not None or c.reduction != "mean" or getattr(c, "label_smoothing", 0.0) != 0.0:
            return None
        if not (hasattr(m, "_native_head") and getattr(m, "native_head", False) and getattr(m, "fuse_pool", False)):
            return None
        if not m._pool_is_global_average() or self.engine.root is not m.features:
            return None
        return m._native_head()

    @property
    def buckets(self):
        return self.schedule.buckets if self.schedule is not None else None

    def sync_buffers(self):
        """Rank-0 BatchNorm running statistics win (DataParallel semantics, train.py:202) -- call before
        validation / checkpointing."""
        if not self.distributed:
            return
        import torch.distributed as dist
        for b in self.model.buffers():
            dist.broadcast(b, src=0, group=self.buckets.group)

    def step(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """One iteration of train.py:427-440.  Returns the loss tensor (no host sync).  ``target``: what the criterion takes -- class
        indices, an (N, C) label matrix (MultiClassBCELoss, MultiLabelLoss), a mixing.MixedTarget (MixCrossEntropyLoss,
        DistillCrossEntropyLoss), a mixing.MixedLabels (MultiLabelLoss) or a losses.DistillTarget (DistillCrossEntropyLoss), on either
        path.  With ``teacher=`` given the teacher's eval forward runs
        first and the target is wrapped into a DistillTarget (:meth:`_teach`)."""
        self._check_target(target)                           # before zero_grad: a refused target leaves the step untouched
        if self.teacher is not None:
            self._check_teacher()
            target = self._teach(x, target)
        self.optimizer.zero_grad()                           # train.py:438
        if self.schedule is not None:
            eng = self.engine
            self.schedule.begin_step(eng.step_stage(eng.first_trainable_step()))
        loss = self.forward_backward(x, target)
        if self.schedule is not None:
            self.schedule.finish()
        self.optimizer.step()                                # train.py:440
        return loss

    def forward_backward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """train.py:427-439 without the optimizer: forward, loss, backward INTO the flat gradient buffer (accumulating into what is
        already there: two calls between ``optimizer.zero_grad()`` and ``optimizer.step()`` sum their gradients, which is what
        the world-2 test uses to emulate two data-parallel ranks in one process).  Fires the engine's stage-done callback."""
        from .losses import DistillTarget
        from .mixing import MixedLabels, MixedTarget
        self._check_meters(self.meters)                      # before any launch, on either path
        self._check_target(target)
        head = self._native_head()
        if head is not None:
            # features -> pool -> head -> cross-entropy -> head backward -> features backward as plain launch lists: no
            # autograd graph, no ATen kernels (csrc/mnas_head.hip); same arithmetic as the module path below
            eng = self.engine
            if hasattr(self.model, "_sync_input_norm"):
                self.model._sync_input_norm()
            eng.check_input(x)                               # same checks as Engine.forward: the launch lists take raw pointers
            if not isinstance(target, (torch.Tensor, MixedTarget, MixedLabels, DistillTarget)) or target.device != x.device:
                raise RuntimeError("target must be a tensor on the input's device (%s)" % (x.device,))
            u8 = x.dtype == torch.uint8 and eng._in_norm is not None
            x = x.contiguous() if u8 else x.float().contiguous()
            eng.ensure_setup(x.device)
            eng._check_modes()
            prog = eng.program(x.shape[0], x.shape[2], x.shape[3], True, False, True, u8, frozen_bn=not eng.root.training,
                               first_trainable=self._frozen_prefix())
            f = prog.run_forward(x, static_io=True)
            head.calls = self.optimizer.step_count           # dropout masks follow the CHECKPOINTED step count: a resumed run does
                                                             # not replay the masks of the first steps
            # with meters: the loss kernels also rank every row's target and move the meters block -- no launch more
            if self._multilabel() or self._mlloss():
                # (a MultiLabelLoss: also a MixedLabels, counted against each row's dominant image)
                # train.py:429 target.float(); the meters' weights are the reference's: input.size(0) for the loss and Dice,
                # input.size(1) for F1 (train.py:447, 454, 463)
                self.last_logits, loss, df = head.loss_and_grad(f.view(f.size(0), -1), target, meters=self._ml_meters(),
                                                                criterion=self.criterion, f1_n=x.shape[1])
            else:                                            # (a MixCrossEntropyLoss: its smoothing and a MixedTarget's two labels; a
                                                             # DistillCrossEntropyLoss: also its weights and a DistillTarget's logits)
                self.last_logits, loss, df = head.loss_and_grad(f.view(f.size(0), -1), target, self.criterion.ignore_index,
                                                                meters=self.meters, criterion=self.criterion)
            accumulate = eng.prepare_grads()
            prog.run_backward(df, eng.on_stage_done, static_io=True)
            eng.finish_grads(accumulate)
        else:
            out = self.model(x.float())
            loss = self.criterion(out, target)
            loss.backward()
            if isinstance(target, DistillTarget):
                target = target.target                       # the meters count the labels
            if isinstance(target, MixedLabels):
                target = target.dominant()                   # the meters count the labels of the image with the larger weight
            if self._ml_meters() is not None:
                if self._label_matrix(out, target):
                    self.meters.update(out.detach(), target, loss.detach(), f1_n=x.shape[1])
            elif self.meters is not None and isinstance(target, MixedTarget):
                self.meters.update(out.detach(), target.dominant(), loss.detach())      # the label with the larger weight
            elif self.meters is not None and self._class_vector(out, target):
                self.meters.update(out.detach(), target, loss.detach())
        return loss.detach()

    def _ml_meters(self):
        """self.meters when it is a MultiLabelMeters, else None (_check_meters has settled that the kind fits the criterion)"""
        from .metrics import MultiLabelMeters
        return self.meters if isinstance(self.meters, MultiLabelMeters) else None

    @staticmethod
    def _label_matrix(out, target):
        """multi-label classification: (N, C) outputs and an (N, C) target on the same device"""
        return isinstance(target, torch.Tensor) and out.dim() == 2 and target.shape == out.shape and target.device == out.device

    @staticmethod
    def _class_vector(out, target):
        """single-label classification: (N, C) outputs and an int64 class index per row (what the meters count)"""
        return (isinstance(target, torch.Tensor) and target.dtype == torch.int64 and out.dim() == 2 and target.shape == (out.shape[0],)
                and target.device == out.device)

    def validate(self, batches, meters=None, transform=None, max_batches=None, reduce=True):
        """The reference's validate() (train.py:556-592) with its three host reads per batch replaced by ONE at the end.

        ``model.eval()`` and ``torch.no_grad()``; for every ``(input, target)`` of ``batches``: ``transform(input)`` if given (a
        transforms.DevicePipeline / DeviceTransform over an ImageBatch), the engine's eval-mode forward with the fused pool, the
        native head without dropout, and the cross-entropy kernels that also move ``meters`` (default: a fresh DeviceMeters with
        top-1 / top-5).  With this package's MultiClassBCELoss as the criterion it is the multi-label pass (train.py:575-587): (N, C)
        targets, the BCE kernels, and a MultiLabelMeters (loss, HardDice(0.5), macro-F1; the default is a fresh one); with its
        MultiLabelLoss the same pass with that loss, on plain label matrices.  With this package's
        MixCrossEntropyLoss it is the single-label pass with the smoothed loss, on plain int64 targets; with its DistillCrossEntropyLoss
        the hard term alone (class weights and smoothing applied; there is no teacher in validation).  Any input shape works: the engine keeps one eval program per shape.  A model or criterion the native head
        does not cover runs as ``model(x)`` / ``criterion`` / ``meters.update``.  Distributed trainers broadcast rank 0's
        BatchNorm statistics first and sum the meters over the ranks at the end (``reduce=False``: neither).  The modules'
        train/eval flags are restored on the way out, also when a batch raises.  Returns ``meters.read()``.  The same pass under the
        EMA weights: :meth:`validate_ema`."""
        from .metrics import DeviceMeters, MultiLabelMeters
        multilabel, mlloss = self._multilabel(), self._mlloss()
        if meters is None:
            meters = MultiLabelMeters(self.device) if multilabel or mlloss else DeviceMeters((1, 5), self.device)
        self._check_meters(meters)
        model = self.model
        modes = [(mod, mod.training) for mod in model.modules()]
        if self.distributed and reduce:
            self.sync_buffers()
        try:
            model.eval()                                                   # train.py:556
            head = self._native_eval_head()
            if head is not None and (model.features._forward_hooks or model.features._forward_pre_hooks
                                     or model.pooling._forward_hooks or model.pooling._forward_pre_hooks):
                head = None                                                # hooks on features / pooling must fire: model(x)
            with torch.no_grad():                                          # train.py:560
                for i, (x, target) in enumerate(batches):
                    if max_batches is not None and i >= max_batches:
                        break
                    if transform is not None:
                        x = transform(x)
                    if not isinstance(target, torch.Tensor) or target.device != x.device:
                        raise RuntimeError("target must be a tensor on the input's device (%s)" % (x.device,))
                    if head is not None:
                        model._sync_input_norm()
                        f = self.engine.forward(x, pooled=True)
                        _, logits = head.forward_layers(f.view(f.size(0), -1), [0] * len(head.layers))   # eval: the seeds are unused
                        if multilabel:                                     # train.py:575-587: weights N, N and input.size(1)
                            head.bce(logits, target, self.criterion, need_grad=False, meters=meters, f1_n=x.shape[1])
                        elif mlloss:                                       # the same pass with this loss, on plain label matrices
                            head.mlabel(logits, target, self.criterion, need_grad=False, meters=meters, f1_n=x.shape[1])
                        elif self._mixce():                                # the smoothed loss on plain class indices
                            head.cross_entropy_soft(logits, target, self.criterion.label_smoothing, self.criterion.ignore_index,
                                                    need_grad=False, meters=meters)
                        elif self._distill():                              # the hard term: weights and smoothing, no teacher
                            head.cross_entropy_kd(logits, target, self.criterion, need_grad=False, meters=meters)
                        else:
                            head.cross_entropy(logits, target, self.criterion.ignore_index, need_grad=False, meters=meters)
                    else:
                        out = model(x)                                     # the engine converts (train.py:562 input.float())
                        loss = self.criterion(out, target)
                        if isinstance(meters, MultiLabelMeters):
                            if not self._label_matrix(out, target):
                                raise ValueError("MultiLabelMeters count multi-label classification: (N, C) targets")
                            meters.update(out, target, loss, f1_n=x.shape[1])
                            continue
                        if not self._class_vector(out, target):
                            raise ValueError("validate() counts single-label classification only: int64 targets of shape (N,)")
                        meters.update(out, target, loss)
        finally:
            for mod, flag in modes:
                mod.training = flag
        if self.distributed and reduce:
            meters.all_reduce(self.buckets.group)
        return meters.read()
