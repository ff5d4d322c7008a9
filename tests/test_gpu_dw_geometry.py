"""-m gpu: the stride-1 depthwise sweeps (k_dw_fwd, k_dw_bwd) at every reachable launch geometry (tests/dw_geometry.py).

Per case -- one launch form at one geometry, row class and set of grids -- the launch runs in every form the ABI offers for it
(virtual and materialised input, with and without the fused reduce, raw and masked g, bias / stats NULL once per k):
  dense    every output and input-gradient element under check_dw_bound, the sums under check_stats_bound / check_sum_bound (c = 2)
           / check_red_bound, all buffers guarded; out / gin bit-identical on a second grid, g_masked bit-identical to raw g; a grid
           below the channel-block count refused with nothing written;
  sparse   the same geometry with a handful of live pixels (dw_geometry.probe_pixels), where the sum bounds are a few 1e-5 of ONE
           product: a dropped, doubled or misplaced strip shows;
  columns  every column of the stats / reduce tables and every row of wpartial against the fp64 sum over exactly the items the
           documented item order gives that workgroup (dw_geometry.column_items): what sees a workgroup that xcd_remap mis-maps;
  stale    the forward / fused-backward launch again, directly after a device-filling launch of another geometry that leaves the
           quiet-NaN pattern 0x7FC0 in the LDS of every CU it ran on: bit-identical results.  Best effort -- where a workgroup lands
           is the hardware's choice, so this can show a read of stale LDS but cannot prove there is none.
tests/test_dw_geometry_cpu.py shows on the CPU that these checks reject the fault of each guard."""
import ctypes as C

import pytest
import torch

import dw_geometry as DG
import intervals
from gpu_util import _FILL, _RAW, L, act_in, bits_equal, grad_in, guarded, pack

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [DG.case_id(c) for c in DG.CASES]
ONCE_PER_K = {k: next(c for c in DG.CASES if c.k == k and c.which == 0 and c.H > 2) for k in (3, 5)}     # bias = NULL and stats = NULL


def _dev(o):
    d = {}
    for name in ("x", "g", "y"):
        if o.get(name) is not None:
            d[name] = o[name].to(torch.bfloat16).to(DEV)
    for name in ("bx", "b", "bi", "bias"):
        d[name] = None if o.get(name) is None else o[name].to(DEV)
    d["wp"] = pack(o["w"].view(o["w"].shape[0], 1, o["w"].shape[1], o["w"].shape[2]), L.PACK_DW)
    return d


def _untouched(t):
    return bool((t.contiguous().view(_RAW[t.element_size()]) == _FILL[t.element_size()]).all())


def _fwd(c, d, nparts, virt=True, bias=True, stats=True, expect=0):
    lib = L.load()
    rows = lib.mnas_dw_rows(c.N, c.H, c.W, c.C, c.k, nparts, 0)
    out, ochk = guarded((c.N, c.H, c.W, c.C), torch.bfloat16)
    st, schk = guarded((2, c.C, max(rows, 1)), torch.float32)
    f = L.MnasDwFwd()
    f.N, f.H, f.W, f.C, f.k, f.nparts = c.N, c.H, c.W, c.C, c.k, nparts
    f.in_ = act_in(d["x"], d["bx"][0], d["bx"][1]) if virt else act_in(d["x"])
    f.w, f.bias, f.out, f.stats = L.ptr(d["wp"]), L.ptr(d["bias"] if bias else None), L.ptr(out), L.ptr(st if stats else None)
    rc = lib.mnas_dw_fwd(C.byref(f), L.cur_stream())
    what = "dw_fwd %s nparts %d%s%s%s" % (DG.case_id(c), nparts, "" if virt else " plain", "" if bias else " no bias", "" if stats else " no stats")
    if expect:
        assert rc == expect and rows == -1, (what, rc, rows)
        ochk(what, written=False)
        schk(what, written=False)
        assert _untouched(out) and _untouched(st), what + ": a refused launch wrote"
        return None
    L.check(rc, what)
    ochk(what + " out")
    schk(what + " stats", written=stats)
    assert stats or _untouched(st), what
    return dict(out=out, stats=st if stats else None, rows=rows, what=what)


def _bwd(c, d, nparts, virt=True, red=True, masked=False, expect=0):
    """generalises test_gpu_bwd_forms._dw_launch to the three phases: a table the phase does not write stays untouched"""
    lib = L.load()
    k, phase = c.k, c.which - 1
    DGr, WG = phase != 2, phase != 1
    rows = lib.mnas_dw_rows(c.N, c.H, c.W, c.C, k, nparts, c.which)
    gin, gchk = guarded((c.N, c.H, c.W, c.C), torch.bfloat16)
    wpart, wchk = guarded((max(rows, 1), k * k, c.C), torch.float32)
    redp, rchk = guarded((2, c.C, max(rows, 1)), torch.float32)
    red = red and DGr
    bn = d["bx"] if virt else d["bi"]
    g = d["gm"] if masked else d["g"]
    a = L.MnasDwBwd()
    a.N, a.H, a.W, a.C, a.k, a.nparts = c.N, c.H, c.W, c.C, k, nparts
    a.x = act_in(d["x"], bn[0], bn[1]) if virt else act_in(d["x"])
    a.dy = grad_in(g, d["y"], d["b"])
    a.w, a.gin, a.wpartial = L.ptr(d["wp"]), L.ptr(gin), L.ptr(wpart)
    if red:
        a.red_bn, a.red_partial = L.ptr(bn), L.ptr(redp)
    a.phase, a.g_masked = phase, 1 if masked else 0
    rc = lib.mnas_dw_bwd(C.byref(a), L.cur_stream())
    what = "dw_bwd %s nparts %d%s%s%s" % (DG.case_id(c), nparts, "" if virt else " plain", " red" if red else "", " g_masked" if masked else "")
    if expect:
        assert rc == expect and rows == -1, (what, rc, rows)
        for chk, t in ((gchk, gin), (wchk, wpart), (rchk, redp)):
            chk(what, written=False)
            assert _untouched(t), what + ": a refused launch wrote"
        return None
    L.check(rc, what)
    gchk(what + " gin", written=DGr)
    wchk(what + " wpartial", written=WG)
    rchk(what + " red_partial", written=red)
    assert (DGr or _untouched(gin)) and (WG or _untouched(wpart)) and (red or _untouched(redp)), what + ": a table of another phase written"
    grad = None
    if WG:
        grad, chk = guarded((c.C, k, k), torch.float32)
        L.check(lib.mnas_dw_wgrad_finalize(L.ptr(wpart.clone()), rows, c.C, k, L.ptr(grad), 0, L.cur_stream()))   # (in place past 256 rows)
        chk(what + " dW")
    return dict(gin=gin if DGr else None, wpart=wpart if WG else None, red=redp if red else None, rows=rows, grad=grad, what=what)


_POISON = {}


def _poison():
    """a device-filling forward launch of another geometry over a plain input of the bf16 pattern 0x7FC0 (quiet NaN): every ring row
    of every workgroup's LDS holds the pattern afterwards.  Output to a scratch buffer; 4096 items on 1024 workgroups."""
    if not _POISON:
        N, H, W, C_, k = 1024, 4, 32, 192, 3
        x = torch.full((N, H, W, C_), 0x7FC0, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        w = torch.ones(C_, 1, k, k)
        _POISON.update(x=x, wp=pack(w, L.PACK_DW), out=torch.empty_like(x), dims=(N, H, W, C_, k))
    N, H, W, C_, k = _POISON["dims"]
    f = L.MnasDwFwd()
    f.N, f.H, f.W, f.C, f.k, f.nparts = N, H, W, C_, k, 1024
    f.in_ = act_in(_POISON["x"])
    f.w, f.out = L.ptr(_POISON["wp"]), L.ptr(_POISON["out"])
    L.check(L.load().mnas_dw_fwd(C.byref(f), L.cur_stream()), "poison launch")


def _same(a, b, keys, what):
    for key in keys:
        if a.get(key) is not None:
            bits_equal(a[key], b[key], "%s: %s" % (what, key))


def _assert_geometry(c, geo):
    """the launch has the geometry, the row class and the grid classes the table stands for -- asked of the library itself"""
    lib = L.load()
    out = (C.c_int * 7)()
    assert lib.mnas_dw_geometry(c.N, c.H, c.W, c.C, c.k, c.which, out) == 0
    rings = (1, 3, 2, 3)[c.which]
    assert tuple(out) == (geo.cpw, geo.sx, geo.threads, geo.strips, geo.cblocks, rings * 2 * geo.G * geo.rc * 16, geo.G), tuple(out)
    assert geo.threads == 64 * geo.nwaves <= 256 and geo.sx * geo.cpw <= geo.threads and geo.nb <= 2 * geo.nwaves
    nsteps = -(-(c.H + 2 * (c.k // 2)) // geo.G)
    assert ("single step" in DG.row_classes(c.H, c.k, geo.G)) == (nsteps == 1)
    for n in c.nparts:
        geff, items = DG.grid(geo, c.N, n)
        assert lib.mnas_dw_rows(c.N, c.H, c.W, c.C, c.k, n, c.which) == (geff // geo.cblocks if geff else -1), n
        assert geff % geo.cblocks == 0 and geff <= min(n, items)


@pytest.mark.parametrize("c", DG.CASES, ids=IDS)
def test_dw_geometry_case(c):
    geo = DG.case_geo(c)
    _assert_geometry(c, geo)
    valid, refused = DG.case_grids(c)
    fwd = c.which == 0
    launch = _fwd if fwd else _bwd

    def check(refs, r, n, dense=True, virt=True, bias=True):
        if fwd:
            DG.check_fwd(c, geo, refs, r, n, virt, bias, r["what"], dense)
        else:
            DG.check_bwd(c, geo, refs, r, n, virt, r["grad"], r["what"], dense)
        if not dense:
            DG.check_sparse(c, geo, refs, r, None if fwd else r["grad"], r["what"])

    # ---- dense
    o = DG.dense_operands(c)
    refs = DG.Refs(c, geo, o, DEV)
    d = _dev(o)
    if not fwd:
        mask = (d["b"][0].double() * d["y"].double() + d["b"][1].double()) > 0
        d["gm"] = torch.where(mask, d["g"], torch.zeros_like(d["g"]))
    n0 = valid[0]
    first = launch(c, d, n0)
    check(refs, first, n0)
    for n in valid[1:]:                                    # other grids: out / gin must not depend on nparts, the tables have their own columns
        r = launch(c, d, n)
        _same(first, r, ("out", "gin"), r["what"] + " against nparts %d" % n0)
        check(refs, r, n)
    for n in refused:
        launch(c, d, n, expect=L.EINVAL)
    if fwd:
        check(refs, _fwd(c, d, n0, virt=False), n0, virt=False)
        if c is ONCE_PER_K[c.k]:
            r = _fwd(c, d, n0, bias=False, stats=False)
            check(refs, r, n0, bias=False)
    else:
        if c.which == 1:
            r = _bwd(c, d, n0, masked=True)
            _same(first, r, ("gin", "wpart", "red"), r["what"] + " against raw g")
        if c.which in (1, 2):
            check(refs, _bwd(c, d, n0, red=False), n0)
        if c.which in (1, 3):
            check(refs, _bwd(c, d, n0, virt=False, red=False), n0, virt=False)
    # ---- stale LDS (best effort): the same launch directly after a device-filling launch that leaves NaN patterns in the rings
    if c.which in (0, 1):
        _poison()
        r = launch(c, d, n0)
        _same(first, r, ("out", "stats", "gin", "wpart", "red"), r["what"] + " after a device-filling launch of another geometry")
    # ---- sparse probe of the same geometry, on every grid
    s = DG.sparse_operands(c, geo)
    srefs = DG.Refs(c, geo, s, DEV, exact=True)
    sd = _dev(s)
    for n in valid:
        r = _fwd(c, sd, n, virt=False, bias=False) if fwd else _bwd(c, sd, n)
        check(srefs, r, n, dense=False, virt=not fwd, bias=False)


def test_dw_geometry_report():
    """worst measured error / bound per launch form and quantity over the cases above (a measurement)"""
    for fam in sorted(f for f in intervals.WORST if f.startswith("dw geometry")):
        print("%-48s %.4f" % (fam, intervals.WORST[fam]))
