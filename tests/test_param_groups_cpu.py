"""CPU (no GPU needed): the table builder of the grouped optimizer steps, the groups on the real model, every refusal of the Python
layer and of the three mnas_*_step_seg entry points, the ctypes mirrors against the header, the state dict with several groups, the
numpy reference (tests/groups_ref.py) against torch.optim.AdamW, and the width of the trust-ratio hulls on the GPU tests' data."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bounds_groups as BG
import groups_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_tables(ranges, rg, gi, tb, tile):
    covered = np.zeros(ranges[-1][1], dtype=np.int64)
    for (begin, n, seg) in tb.tiles:
        assert 1 <= n <= tile
        sb, sn = tb.segs[seg][:2]
        assert sb <= begin and begin + n <= sb + sn                      # inside ONE segment
        covered[begin:begin + n] += 1
    want = np.zeros_like(covered)
    for (a, b), r in zip(ranges, rg):
        if r:
            want[a:b] = 1
    assert np.array_equal(covered, want)                                 # exact cover of the trainable elements, no overlap
    k = 0
    for (begin, n, group, t0, nt, param) in tb.segs:
        assert ranges[param] == (begin, begin + n) and rg[param] and group == gi[param]
        assert t0 == k and nt == -(-n // tile)                           # consecutive tiles, in element order
        assert [t[0] for t in tb.tiles[t0:t0 + nt]] == [begin + j * tile for j in range(nt)]
        assert all(t[2] == tb.segs.index((begin, n, group, t0, nt, param)) for t in tb.tiles[t0:t0 + nt])
        k += nt
    assert k == len(tb.tiles)


def test_table_builder():
    from mnasnet_pytorch_amd import _lib
    from mnasnet_pytorch_amd.train_step import build_opt_tables
    lay = BG.standard_layout()
    tb = build_opt_tables(*lay)
    assert _lib.OPT_TILE == 4096 and len(tb.segs) == 9 and lay[0][-1][1] == 29967
    assert [s[1] for s in tb.segs] == BG.SIZES and [s[2] for s in tb.segs] == [0, 1, 2] * 3
    assert [s[4] for s in tb.segs] == [1, 1, 1, 1, 1, 1, 1, 2, 3]
    assert BG.FROZEN_AT not in [s[5] for s in tb.segs]                   # the frozen tensor has no segment
    _check_tables(*lay, tb, 4096)
    # another tile size, an empty tensor, everything frozen
    ranges = [(0, 10), (10, 10), (10, 31), (31, 32)]
    tb = build_opt_tables(ranges, [True, True, True, False], [1, 0, 0, 1], tile=8)
    assert [s[:5] for s in tb.segs] == [(0, 10, 1, 0, 2), (10, 21, 0, 2, 3)] and len(tb.tiles) == 5
    _check_tables(ranges, [True, False, True, False], [1, 0, 0, 1], tb, 8)
    assert build_opt_tables(ranges, [False] * 4, [0] * 4) == ([], [])
    many = BG.many_layout()
    tb = build_opt_tables(*many)
    assert len(tb.segs) == len(tb.tiles) == 2100 > 2048
    _check_tables(*many, tb, 4096)


def _cpu_params(sizes):
    n = sum(sizes)
    flat_p, flat_g = torch.arange(n, dtype=torch.float32), torch.zeros(n)
    out, off = [], 0
    for k in sizes:
        par = torch.nn.Parameter(flat_p[off:off + k])
        par.data = flat_p[off:off + k]
        out.append(par)
        off += k
    return out, flat_p, flat_g


def test_tables_follow_requires_grad_and_membership():
    from mnasnet_pytorch_amd.train_step import FlatAdam
    ps, flat_p, flat_g = _cpu_params([5, 3, 9000, 2])
    opt = FlatAdam([{"params": [ps[0], ps[2]]}, {"params": [ps[3], ps[1]], "weight_decay": 0.0}], flat_p, flat_g, weight_decay=0.1)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0] and opt._grouped()
    assert opt._ranges == [(0, 5), (5, 8), (8, 9008), (9008, 9010)] and opt._trainable_runs() == [[0, 9010]]
    first = opt._seg_tables()
    assert [s[:3] for s in first["tables"].segs] == [(0, 5, 0), (5, 3, 1), (8, 9000, 0), (9008, 2, 1)]
    assert opt._seg_tables() is first                                    # nothing changed: not rebuilt
    ps[1].requires_grad_(False)
    second = opt._seg_tables()
    assert second is not first and [s[5] for s in second["tables"].segs] == [0, 2, 3]
    assert opt._trainable_runs() == [[0, 5], [8, 9010]]
    moved = opt.param_groups[1]["params"].pop(0)                         # membership: a tensor moves to the other group
    assert moved is ps[3]
    opt.param_groups[0]["params"].append(moved)
    third = opt._seg_tables()
    assert third is not second and [s[2] for s in third["tables"].segs] == [0, 0, 0]
    assert opt.param_groups[0]["params"].pop() is ps[3]
    with pytest.raises(ValueError, match="every parameter"):
        opt._seg_tables()


@pytest.mark.parametrize("decoupled", [False, True])
def test_one_dict_group_in_another_order_than_the_addresses(decoupled):
    """A group dict may list its parameters in any order (torch's model.parameters() yields the features first, the flat buffer
    holds the head first).  The element ranges are in address order, so the trainable runs -- the plain launches' and the global
    norm's -- and the segment table must be too: tensors of 4, 6 and 2 elements handed over reversed, the first (by address) frozen."""
    from mnasnet_pytorch_amd.train_step import FlatAdam, FlatRMSprop, FlatSGD
    for cls in (FlatAdam, FlatRMSprop, FlatSGD):
        ps, flat_p, flat_g = _cpu_params([4, 6, 2])
        opt = cls([{"params": [ps[2], ps[1], ps[0]]}], flat_p, flat_g, decoupled_weight_decay=decoupled)
        assert opt._grouped() == decoupled and opt._ranges == [(0, 4), (4, 10), (10, 12)]
        assert [id(p) for p in opt._all_params] == [id(p) for p in ps]
        assert opt._trainable_runs() == [[0, 12]]
        ps[0].requires_grad_(False)
        assert opt._trainable_runs() == [[4, 12]]
        assert [s[:3] + s[5:] for s in opt._seg_tables()["tables"].segs] == [(4, 6, 0, 1), (10, 2, 0, 2)]
        ps[0].requires_grad_(True)
        ps[1].requires_grad_(False)
        assert opt._trainable_runs() == [[0, 4], [10, 12]]
        assert [s[:3] + s[5:] for s in opt._seg_tables()["tables"].segs] == [(0, 4, 0, 0), (10, 2, 0, 2)]
        sd = opt.state_dict()
        assert sd["param_groups"][0]["params"] == [0, 1, 2]


def test_groups_on_the_real_model():
    from mnasnet_pytorch_amd import FineTuneModelPool, Mnasnet
    from mnasnet_pytorch_amd.train_step import build_opt_tables, norm_bias_groups, stage_lr_groups
    feats = list(Mnasnet(cut_channels_first=False).features.parameters())
    assert len(feats) == 108 and sum(p.ndim <= 1 for p in feats) == 81
    m = FineTuneModelPool(Mnasnet(cut_channels_first=False), "mnasnet", 10, "512")
    groups = norm_bias_groups(m, 1e-5)
    head_bias = [p for p in m.classifier.parameters() if p.ndim == 1]
    assert len(head_bias) == 2 and len(groups) == 2
    assert groups[0]["weight_decay"] == 1e-5 and groups[1]["weight_decay"] == 0.0 and groups[1]["trust"] is False
    assert len(groups[1]["params"]) == 81 + 2 and {id(p) for p in head_bias} <= {id(p) for p in groups[1]["params"]}
    assert all(p.ndim <= 1 for p in groups[1]["params"]) and all(p.ndim > 1 for p in groups[0]["params"])
    assert len(groups[0]["params"]) + len(groups[1]["params"]) == len(list(m.parameters())) == 112
    # one segment per feature tensor
    sizes = [p.numel() for p in feats]
    ranges = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
    tb = build_opt_tables(ranges, [True] * 108, [int(p.ndim <= 1) for p in feats])
    assert len(tb.segs) == 108 and sum(s[2] for s in tb.segs) == 81 and len(tb.tiles) == sum(-(-k // 4096) for k in sizes)
    # layer-wise rates: the head at lr, features[k] at lr * decay^(7 - k); composed with the first helper: every key survives
    st = stage_lr_groups(m, 0.1, 0.5)
    assert len(st) == 9 and st[0]["lr"] == 0.1 and {id(p) for p in st[0]["params"]} == {id(p) for p in m.classifier.parameters()}
    assert [g["lr"] for g in st[1:]] == [0.1 * 0.5 ** j for j in range(8)]
    assert {id(p) for p in st[-1]["params"]} == {id(p) for p in m.features[0].parameters()}
    both = stage_lr_groups(m, 0.1, 0.5, norm_bias_groups(m, 1e-5))
    assert len(both) == 18 and sum(len(g["params"]) for g in both) == 112
    assert sorted({g["weight_decay"] for g in both}) == [0.0, 1e-5] and sum("trust" in g for g in both) == 9


@pytest.mark.parametrize("kind", ["adam", "rmsprop", "sgd"])
def test_refusals_before_any_launch(kind):
    from mnasnet_pytorch_amd import _lib
    from mnasnet_pytorch_amd.train_step import FlatAdam, FlatRMSprop, FlatSGD
    cls = {"adam": FlatAdam, "rmsprop": FlatRMSprop, "sgd": FlatSGD}[kind]
    ps, flat_p, flat_g = _cpu_params([4, 6, 2])
    with pytest.raises(ValueError, match="more than one"):
        cls([{"params": [ps[0], ps[1]]}, {"params": [ps[1], ps[2]]}], flat_p, flat_g)
    with pytest.raises(ValueError, match="tile flat_p"):
        cls([{"params": [ps[0]]}, {"params": [ps[2]]}], flat_p[:6], flat_g[:6])             # a hole where ps[1] is
    with pytest.raises(ValueError, match="exactly the parameters"):
        cls([{"params": [ps[0], ps[1]]}], flat_p, flat_g)
    many = _cpu_params([1] * (_lib.OPT_MAX_GROUPS + 1))
    with pytest.raises(ValueError, match="MNAS_OPT_MAX_GROUPS"):
        cls([{"params": [p]} for p in many[0]], many[1], many[2])
    with pytest.raises(ValueError, match="trust_ratio"):
        cls(ps, flat_p, flat_g, trust_ratio="lion")
    wrong = {"adam": "lars", "rmsprop": "lamb", "sgd": "lamb"}[kind]
    with pytest.raises(ValueError, match="not available"):
        cls(ps, flat_p, flat_g, trust_ratio=wrong)
    if kind == "rmsprop":
        with pytest.raises(ValueError, match="not available"):
            cls(ps, flat_p, flat_g, trust_ratio="lars")
        return
    own = {"adam": "lamb", "sgd": "lars"}[kind]
    with pytest.raises(ValueError, match="exclude each other"):
        cls(ps, flat_p, flat_g, trust_ratio=own, decoupled_weight_decay=True)
    with pytest.raises(ValueError, match="exclude each other"):
        cls([{"params": ps[:2]}, {"params": ps[2:], "decoupled": True}], flat_p, flat_g, trust_ratio=own)
    with pytest.raises(ValueError, match="trust_eps"):
        cls(ps, flat_p, flat_g, trust_ratio=own, trust_eps=-1.0)
    ok = cls([{"params": ps[:2]}, {"params": ps[2:], "decoupled": True, "trust": False}], flat_p, flat_g, trust_ratio=own)
    assert [(g["decoupled"], g["trust"]) for g in ok.param_groups] == [(False, True), (True, False)]
    ok.param_groups[1]["trust"] = True                                   # plain dicts: checked again when a step reads them
    with pytest.raises(ValueError, match="exclude each other"):
        ok.step()
    ok.param_groups[1]["trust"] = False
    ok.param_groups[0]["lr"] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ok.step()
    # the routing: one group without the new options keeps today's path
    plain = cls(ps, flat_p, flat_g)
    assert not plain._grouped() and plain.seg_calls == 0 and plain.trust_ratios() == {} and plain.last_trust_ratios is None
    assert cls(ps, flat_p, flat_g, decoupled_weight_decay=True)._grouped() and cls([{"params": ps[:1]}, {"params": ps[1:]}], flat_p, flat_g)._grouped()


def test_trainer_surface():
    import inspect
    from mnasnet_pytorch_amd import train_step as T
    sig = inspect.signature(T.Trainer.__init__).parameters
    assert sig["param_groups"].default is None and sig["decoupled_weight_decay"].default is False
    assert sig["trust_ratio"].default is None and sig["trust_coef"].default == 1e-3
    for cls in (T.FlatAdam, T.FlatRMSprop, T.FlatSGD):
        s = inspect.signature(cls.__init__).parameters
        if cls is T.FlatAdam:
            assert (s["decoupled_weight_decay"].default, s["trust_ratio"].default, s["trust_coef"].default, s["trust_eps"].default) == \
                (False, None, 1e-3, 1e-8)
    assert hasattr(T.Trainer, "trust_ratios") and callable(T.norm_bias_groups) and callable(T.stage_lr_groups)
    assert "decoupled_weight_decay=True" in T.Trainer.__doc__ and "adamw" in T.Trainer.__doc__


def _c_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([\w ]+?\*?)\s+(\w+);", body)


def test_header_symbols_and_struct_mirrors():
    from mnasnet_pytorch_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mnas.h")).read()
    for name, k in {"mnas_adam_step_seg": 12, "mnas_rmsprop_step_seg": 11, "mnas_sgd_step_seg": 11}.items():
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == k, name
        assert _lib.SYMBOLS[name][1][-3] is ctypes.POINTER(_lib.MnasOptSegs) and _lib.SYMBOLS[name][1][-2] is ctypes.POINTER(_lib.MnasOptExtra)
    assert lib.mnas_version() == _lib.ABI_VERSION == 8                   # additive: the version does not move
    for macro, val in (("MNAS_OPT_TILE", _lib.OPT_TILE), ("MNAS_OPT_MAX_GROUPS", _lib.OPT_MAX_GROUPS), ("MNAS_OPT_MAX_SEGS", _lib.OPT_MAX_SEGS),
                       ("MNAS_TRUST_NONE", _lib.TRUST_NONE), ("MNAS_TRUST_LAMB", _lib.TRUST_LAMB), ("MNAS_TRUST_LARS", _lib.TRUST_LARS)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, hdr).group(1)) == val, macro
    assert (_lib.OPT_TILE, _lib.OPT_MAX_GROUPS, _lib.OPT_MAX_SEGS) == (4096, 32, 4096)
    ctype = {"float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    for name, cls, size in (("MnasOptSeg", _lib.MnasOptSeg, 32), ("MnasOptTile", _lib.MnasOptTile, 16), ("MnasOptGroup", _lib.MnasOptGroup, 16),
                            ("MnasOptSegs", _lib.MnasOptSegs, 64)):
        fields = [(" ".join(t.split()), n) for t, n in _c_fields(hdr, name)]
        assert [n for _, n in fields] == [n for n, _ in cls._fields_], name
        for (t, n), (_, ct) in zip(fields, cls._fields_):
            if t.endswith("*"):
                assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (name, n)
            else:
                assert ct is ctype[t], (name, n)
        assert ctypes.sizeof(cls) == size, name


def test_entry_points_check_their_arguments_on_the_host():
    """Every bad argument is refused on the host, before a launch (null streams; the calls that succeed are empty: nsegs == 0)."""
    from mnasnet_pytorch_amd import _lib
    lib, E = _lib.load(), _lib.EINVAL
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)

    def segs(groups=((1e-3, 0.0, 0, 0),), **kw):
        garr = (_lib.MnasOptGroup * max(1, len(groups or ())))(*[_lib.MnasOptGroup(*g) for g in groups or ()])
        base = dict(segs=a, tiles=a, groups=garr if groups is not None else None, nsegs=0, ntiles=0, ngroups=len(groups or (0,)),
                    trust_kind=0, tile_partial=a, ratio=a,
                    trust_coef=1e-3, trust_eps=1e-8)
        base.update(kw)
        s = _lib.MnasOptSegs(**base)
        s._keep = garr
        return s

    def adam(s, ex=None, p=a, step=1, gscale=1.0):
        return lib.mnas_adam_step_seg(p, a, a, a, 0.9, 0.999, 1e-8, step, gscale, ctypes.byref(s) if s is not None else None, ex, None)

    def rms(s, ex=None, p=a, step=1, gscale=1.0):
        return lib.mnas_rmsprop_step_seg(p, a, a, None, 0.99, 1e-8, 0.0, gscale, ctypes.byref(s) if s is not None else None, ex, None)

    def sgd(s, ex=None, p=a, step=1, gscale=1.0):
        return lib.mnas_sgd_step_seg(p, a, None, 0.0, 0.0, 0, step, gscale, ctypes.byref(s) if s is not None else None, ex, None)

    nan = float("nan")
    for fn in (adam, rms, sgd):
        assert fn(segs()) == 0                                           # valid and empty: no launch
        assert fn(None) == E and fn(segs(), p=None) == E
        assert fn(segs(segs=None)) == E and fn(segs(tiles=None)) == E and fn(segs(groups=None)) == E
        assert fn(segs(nsegs=-1)) == E and fn(segs(nsegs=_lib.OPT_MAX_SEGS + 1, ntiles=_lib.OPT_MAX_SEGS + 1)) == E
        assert fn(segs(ntiles=-1)) == E and fn(segs(nsegs=2, ntiles=1)) == E
        assert fn(segs(ngroups=0)) == E and fn(segs(ngroups=_lib.OPT_MAX_GROUPS + 1)) == E
        assert fn(segs(trust_kind=3)) == E and fn(segs(trust_kind=-1)) == E
        assert fn(segs(groups=((nan, 0.0, 0, 0),))) == E and fn(segs(groups=((1e-3, nan, 0, 0),))) == E
        assert fn(segs(groups=((1e-3, 0.0, 0, 0), (1e-3, 0.1, 1, 1)))) == E             # decoupled and trust in one group
        assert fn(segs(trust_eps=-1e-8)) == E and fn(segs(trust_eps=nan)) == E and fn(segs(trust_coef=nan)) == E
        assert fn(segs(), gscale=nan) == E
        bad = _lib.MnasOptExtra(partial=None, nparts=1, max_norm=1.0, skip_nonfinite=0, ema=None, ema_decay=0.0, stats=a, update_stats=1)
        assert fn(segs(), ex=ctypes.byref(bad)) == E                      # what mnas_*_step_ex refuses of an extra
        good = _lib.MnasOptExtra(partial=a, nparts=1, max_norm=1.0, skip_nonfinite=1, ema=a, ema_decay=0.5, stats=a, update_stats=1)
        assert fn(segs(), ex=ctypes.byref(good)) == 0
    assert adam(segs(), step=0) == E and sgd(segs(), step=0) == E
    assert adam(segs(trust_kind=_lib.TRUST_LAMB)) == 0 and sgd(segs(trust_kind=_lib.TRUST_LARS)) == 0
    assert adam(segs(trust_kind=_lib.TRUST_LARS)) == E and sgd(segs(trust_kind=_lib.TRUST_LAMB)) == E
    assert rms(segs(trust_kind=_lib.TRUST_LAMB)) == E and rms(segs(trust_kind=_lib.TRUST_LARS)) == E
    assert adam(segs(trust_kind=_lib.TRUST_LAMB, ratio=None)) == E and sgd(segs(trust_kind=_lib.TRUST_LARS, tile_partial=None)) == E
    assert adam(segs(tile_partial=None, ratio=None)) == 0                 # no trust ratio: the workspaces may be NULL


@pytest.mark.parametrize("kind", ["adam", "rmsprop", "sgd"])
def test_state_dict_with_groups(kind):
    from mnasnet_pytorch_amd.train_step import FlatAdam, FlatRMSprop, FlatSGD
    cls = {"adam": FlatAdam, "rmsprop": FlatRMSprop, "sgd": FlatSGD}[kind]

    def make(grouped):
        ps, flat_p, flat_g = _cpu_params([4, 6, 2])
        if grouped:
            return cls([{"params": [ps[0], ps[2]], "lr": 0.5}, {"params": [ps[1]], "weight_decay": 0.25, "decoupled": True}], flat_p, flat_g)
        return cls(ps, flat_p, flat_g)

    opt = make(True)
    opt.param_groups[0]["lr"] = 0.125
    opt.flat_m.fill_(2.0)
    opt.step_count = 7
    sd = opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1], [2]]
    assert [(g["lr"], g["weight_decay"], g["decoupled"], g["trust"]) for g in sd["param_groups"]] == \
        [(0.125, 0.0, False, False), (opt.defaults["lr"], 0.25, True, False)]
    other = make(True)
    other.load_state_dict(sd)
    assert other.step_count == 7 and bool((other.flat_m == 2.0).all())
    assert [{k: v for k, v in g.items() if k != "params"} for g in other.param_groups] == \
        [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]
    with pytest.raises(ValueError, match="parameter groups"):
        make(False).load_state_dict(sd)
    # a one-group checkpoint as it was written before the groups existed: no 'decoupled' / 'trust' keys
    single = make(False)
    old = single.state_dict()
    assert len(old["param_groups"]) == 1 and old["param_groups"][0]["params"] == [0, 1, 2]
    for k in ("decoupled", "trust"):
        del old["param_groups"][0][k]
    old["param_groups"][0]["lr"] = 0.75
    old["state"]["step"] = 3
    fresh = make(False)
    fresh.load_state_dict(old)
    assert fresh.param_groups[0]["lr"] == 0.75 and fresh.step_count == 3
    assert fresh.param_groups[0]["decoupled"] is False and fresh.param_groups[0]["trust"] is False and not fresh._grouped()


def test_reference_is_torchs_adamw():
    """groups_ref.adamw_step (float64) against torch.optim.AdamW on float64 CPU tensors, three steps: 1e-12 relative"""
    gen = torch.Generator().manual_seed(2)
    p0 = torch.randn(501, generator=gen, dtype=torch.float64)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    p, m, v = p0.numpy().copy(), np.zeros(501), np.zeros(501)
    for step in (1, 2, 3):
        g = torch.randn(501, generator=gen, dtype=torch.float64)
        ref.grad = g.clone()
        opt.step()
        p, m, v = GR.adamw_step(p, g.numpy(), m, v, 3e-3, 0.9, 0.999, 1e-8, 0.05, step)
    assert np.abs(p - ref.detach().numpy()).max() <= 1e-12 * np.abs(p).max()
    # the rules of the two ratios, at the optimizers' default trust_coef / trust_eps
    import inspect
    from mnasnet_pytorch_amd.train_step import FlatSGD
    sig = inspect.signature(FlatSGD.__mro__[1].__init__).parameters
    coef, eps = sig["trust_coef"].default, sig["trust_eps"].default
    assert (coef, eps) == (1e-3, 1e-8)
    assert GR.lamb_ratio(0.0, 2.0) == 1.0 and GR.lamb_ratio(2.0, 0.0) == 1.0 and GR.lamb_ratio(3.0, 2.0) == 1.5
    assert GR.lars_ratio(0.0, 1.0, 0.1, coef, eps) == 1.0 and GR.lars_ratio(1.0, 0.0, 0.1, coef, eps) == 1.0
    assert abs(GR.lars_ratio(2.0, 1.0, 0.5, coef, eps) - coef) < 1e-10
    assert abs(GR.lars_ratio(2.0, 1.0, 0.5, 0.1, 0.0) - 0.1) < 1e-15
    assert GR.norm([3.0, 4.0]) == 5.0


def test_trust_ratio_hulls_are_narrow():
    """The hull bounds_groups gives un and r on the GPU tests' data is narrower than 2^-10 relative for every tensor that takes a real
    ratio: a bracket that wide would let the GPU test pass vacuously.  Reference data only; nothing of the device."""
    from mnasnet_pytorch_amd.train_step import build_opt_tables
    for name in ("standard", "many"):
        lay = BG.standard_layout() if name == "standard" else BG.many_layout()
        tb = build_opt_tables(*lay)
        st = BG.trust_state(lay, tb) if name == "standard" else BG.flat_state(lay, 9)
        widest, real = 0.0, 0
        for k, (begin, n, gi) in enumerate(s[:3] for s in tb.segs):
            if gi == 2:
                continue                                                 # the trust = False group
            s = BG.slice_state(st, begin, begin + n)
            w_ref = GR.norm(s["p"].numpy())
            u_iv = BG.lamb_direction(s, BG.ADAM, BG.GROUPS3[gi][1])[0]
            gs = (s["g"] * torch.tensor(BG.ADAM["gscale"])).numpy()
            u_ref = GR.lamb_direction(s["p"].numpy(), gs, s["m"].numpy(), s["v"].numpy(), BG.ADAM["b1"], BG.ADAM["b2"], BG.ADAM["eps"],
                                      BG.GROUPS3[gi][1], BG.ADAM["step"])[0]
            if w_ref == 0.0 or GR.norm(u_ref) == 0.0:
                assert name == "many" or k in (BG.ZERO_P_SEG, BG.ZERO_G_SEG)
                continue
            un_lo, un_hi, r_lo, r_hi = BG.lamb_ratio_hull(w_ref, u_iv)
            assert un_lo > 0
            widest = max(widest, (un_hi - un_lo) / un_lo, (r_hi - r_lo) / r_lo)
            real += 1
        print("%s: %d hulls, widest %.3g relative" % (name, real, widest))
        assert real >= 4 and widest < 2.0 ** -10
    assert BG.LARS_RATIO_REL < 2.0 ** -10
