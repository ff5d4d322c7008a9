"""CPU side of the depthwise geometry cases (tests/dw_geometry.py): the table reaches every reachable (form, feature, value)
triple, row class and grid class and holds no case it could lose; the operands each GPU case uploads meet the conditions of the
bound helpers; and the checks of tests/test_gpu_dw_geometry.py bite -- a plain fp32 emulation of every launch form passes them, the
same emulation with the fault of one guard (dw_geometry.FAULTS) does not."""
import pytest
import torch

import dw_geometry as DG
import intervals
from bounds_conv import MAX_ACT_SPLIT, MAX_DY_SPLIT, MAX_HINGE_MOVED, act_interval, dy_interval
from mnasnet_pytorch_amd import _lib as L

SWEEP_W = list(range(1, 65)) + [72, 80, 96, 112, 113, 128, 160, 224]
SWEEP_C = range(8, 2049, 8)
IDS = [DG.case_id(c) for c in DG.CASES]


@pytest.fixture(scope="module")
def sweep():
    """{(W, C, k, which): Geo} over the whole range"""
    return {(W, C_, k, which): DG.geometry(W, C_, k, which) for W in SWEEP_W for C_ in SWEEP_C for k in (3, 5) for which in range(4)}


def test_geometry_does_not_depend_on_n_or_h(sweep):
    keys = sorted(sweep)[::97]
    for i, (W, C_, k, which) in enumerate(keys):
        for N, H in ((1, 1), (1 + i % 300, 1 + (7 * i) % 230), (256, 224)):
            assert DG.geometry(W, C_, k, which, N, H) == sweep[(W, C_, k, which)], (W, C_, k, which, N, H)


def test_cases_reach_every_reachable_triple(sweep):
    assert all(g is not None for g in sweep.values())
    reach = set().union(*(DG.triples(g) for g in sweep.values()))
    forms = {t[0] for t in reach}
    assert forms == {(k, w, 4) for k in (3, 5) for w in range(4)} | {(k, w, 2) for k in (3, 5) for w in (1, 2, 3)}       # forward: G = 4 only
    unreachable = {t for t, _ in DG.UNREACHABLE}
    assert len(unreachable) == len(DG.UNREACHABLE) and all(why for _, why in DG.UNREACHABLE)
    every = {(f, i, v) for f in forms for i in range(len(DG.FEATURES)) for v in (False, True)}
    assert reach | unreachable == every and not (reach & unreachable), (sorted(every - reach - unreachable), sorted(reach & unreachable))
    covered = set().union(*(DG.case_covers(c)[0] for c in DG.CASES))
    assert covered == reach, (sorted(reach - covered), sorted(covered - reach))
    # a second DMA block that holds image data, in every form (dw_geometry.second_block_live: on a narrow image it can hold padding only)
    live = {(DG.form_of(g), DG.EXTRA) for (W, _, _, _), g in sweep.items() if DG.second_block_live(g, W)}
    assert {f for f, _ in live} == forms
    assert set().union(*(DG.case_covers(c)[3] for c in DG.CASES)) == live
    # what UNREACHABLE's reasons rest on: the one geometry of the 3x3 phase-1 launch with 2-row groups
    assert {(g.cpw, g.sx, g.rc, g.nb, g.nwaves) for g in sweep.values() if DG.form_of(g) == (3, 2, 2)} == {(128, 2, 320, 5, 4)}
    assert all(g.iw * g.cpw > 1248 for g in sweep.values() if g.which == 2 and g.G == 2)


def _needed():
    rows, grids = set(), set()
    for c in DG.CASES:
        geo = DG.case_geo(c)
        rows |= {(c.k, geo.G, c.which == 0, lab) for lab in DG.reachable_row_classes(c.k, geo.G)}
        grids |= {(DG.form_of(geo), lab) for lab in DG.GRID_CLASSES}
    return rows, grids


def test_cases_reach_every_row_and_grid_class():
    rows, grids = _needed()
    assert len({(r[0], r[1], r[2]) for r in rows}) == 6 and len({g[0] for g in grids}) == 14
    got_rows = set().union(*(DG.case_covers(c)[1] for c in DG.CASES))
    got_grids = set().union(*(DG.case_covers(c)[2] for c in DG.CASES))
    assert rows <= got_rows, sorted(rows - got_rows)
    assert grids <= got_grids, sorted(grids - got_grids)
    # the row classes that exist at all: a plane no higher than the padding needs k = 5, one step for the whole plane k = 3 with G = 4
    assert {r[:2] for r in rows if r[3] == "1 < H <= PAD"} == {(5, 4), (5, 2)}
    assert {r[:2] for r in rows if r[3] == "single step"} == {(3, 4)}


def test_no_case_can_be_removed():
    """the coverage assertions above fail for the table without any one of its cases"""
    rows, grids = _needed()
    cov = [DG.case_covers(c) for c in DG.CASES]
    reach, live = (set().union(*(x[j] for x in cov)) for j in (0, 3))
    for i, c in enumerate(DG.CASES):
        rest = cov[:i] + cov[i + 1:]
        t, r, g, e = (set().union(*(x[j] for x in rest)) for j in range(4))
        assert not (reach <= t and rows <= r and grids <= g and live <= e), "%s covers nothing of its own" % DG.case_id(c)


def test_grid_model_is_the_librarys():
    """dw_geometry.grid (what the per-column checks rest on) against mnas_dw_rows, for every grid of every case and a sweep of nparts"""
    lib = L.load()
    for c in DG.CASES:
        geo = DG.case_geo(c)
        valid, refused = DG.case_grids(c)
        assert len(valid) >= 2 and len(set(valid + refused)) == len(c.nparts), c
        assert len({DG.grid(geo, c.N, n)[0] for n in valid}) >= 2 or c.N * geo.strips == 1, c          # two different grids to compare
        for n in list(c.nparts) + list(range(1, 70)) + [1024]:
            geff, _ = DG.grid(geo, c.N, n)
            assert lib.mnas_dw_rows(c.N, c.H, c.W, c.C, c.k, n, c.which) == (geff // geo.cblocks if geff else -1), (c, n)
    for n in (1, 5, 8, 9, 23, 64, 1000):
        assert sorted(DG.xcd_remap(b, n) for b in range(n)) == list(range(n))


@pytest.mark.parametrize("c", DG.CASES, ids=IDS)
def test_case_operands_meet_the_helpers_conditions(c):
    """on the very tensors the GPU case uploads: at most 1e-3 of the activations and 2e-2 of dy straddle a bf16 rounding boundary,
    at most 1 % of the elements were moved off the ReLU hinge (off_hinge asserts its share while it builds them)"""
    assert (MAX_ACT_SPLIT, MAX_DY_SPLIT, MAX_HINGE_MOVED) == (1e-3, 2e-2, 1e-2)
    intervals.SHARES.pop("hinge", None)
    o = DG.dense_operands(c)
    assert intervals.SHARES.get("hinge", 0.0) <= MAX_HINGE_MOVED
    assert act_interval(o["x"], o["bx"][0], o["bx"][1], True).split_share() <= MAX_ACT_SPLIT
    assert dy_interval(o["g"], o["y"], o["b"], True).split_share() <= MAX_DY_SPLIT
    geo = DG.case_geo(c)
    s = DG.sparse_operands(c, geo)
    M = c.N * c.H * c.W
    live = s["x"] if c.which == 0 else s["g"]
    on = live.view(M, c.C).abs().sum(1) > 0
    assert sorted(int(i) for i in on.nonzero().view(-1)) == s["px"] and 0 < len(s["px"]) <= M
    assert bool((live.view(M, c.C)[s["px"]] != 0).all())                              # live channels are dense
    tw = 4 * geo.sx
    for st in range(1, geo.strips):                                                    # both sides of EVERY strip boundary
        assert any(p % c.W == st * tw - 1 for p in s["px"]) and any(p % c.W == st * tw for p in s["px"])
    assert any(p % c.W == c.W - 1 and p // c.W % c.H == c.H - 1 for p in s["px"])


def _check(c, geo, refs, res, n, dense, what):
    if c.which == 0:
        DG.check_fwd(c, geo, refs, res, n, dense, dense, what, dense)
        grad = None
    else:
        grad = None if res["wpart"] is None else res["wpart"].double().sum(0).float().t().reshape(c.C, c.k, c.k)
        DG.check_bwd(c, geo, refs, res, n, True, grad, what, dense)
    if not dense:
        DG.check_sparse(c, geo, refs, res, grad, what)


@pytest.mark.parametrize("c", DG.CASES, ids=IDS)
def test_checks_admit_the_emulation_and_reject_each_fault(c):
    """The emulation is fp32 torch on the CPU (conv2d per item, sums in the kernels' table layout): it must pass the dense and the
    sparse checks on every grid of the case.  Then, per fault the case's geometry carries: the faulty emulation is rejected by the
    dense or by the sparse check.  Two workgroups' table columns swapped change no sum: only the per-column check sees them."""
    geo = DG.case_geo(c)
    dense, sparse = DG.dense_operands(c), DG.sparse_operands(c, geo)
    runs = ((True, dense, DG.Refs(c, geo, dense, "cpu")), (False, sparse, DG.Refs(c, geo, sparse, "cpu", exact=True)))
    valid, _ = DG.case_grids(c)

    def emu(is_dense, o, n, fault=None):
        return DG.emulate(c, geo, o, n, virt=(is_dense or c.which != 0), fault=fault)

    for n in valid:
        for is_dense, o, refs in runs:
            _check(c, geo, refs, emu(is_dense, o, n), n, is_dense, "%s nparts %d" % (DG.case_id(c), n))
    tried = 0
    for fault in DG.FAULTS:
        n = next((n for n in valid if DG.fault_applies(fault, c, geo, n)), None)
        if n is None:
            continue
        tried += 1
        caught = []
        for is_dense, o, refs in runs:
            try:
                _check(c, geo, refs, emu(is_dense, o, n, fault), n, is_dense, "fault")
            except AssertionError as e:
                caught.append(str(e))
                break
        assert caught, "%s: neither the dense nor the sparse check rejects %s at nparts %d" % (DG.case_id(c), fault, n)
        if fault == "col_swap":
            assert "by table" in caught[0], caught[0]
    assert tried >= 2
