"""The stride-1 depthwise sweeps (csrc/mnas_dw.hip: k_dw_fwd, k_dw_bwd) by launch GEOMETRY rather than by template instance.

The host searches the geometry at run time (dw_pick / dw_choose / dw_finish); mnas_dw_geometry and mnas_dw_rows answer for it.  It
depends on (W, C, k, which) only -- N and H never change it (asserted over the sweep of tests/test_dw_geometry_cpu.py).  `which` as
in mnas_dw_rows: 0 forward, 1 / 2 / 3 = backward phase 0 (fused) / 1 (input gradient) / 2 (weight gradient).

  form         (k, which, G): kernel size, launch form, rows per DMA group
  feature      eight yes/no properties of the geometry, each guarded by its own line of the kernels (FEATURES)
  triple       (form, feature index, value): what the case table has to reach, every reachable one (UNREACHABLE lists the rest)
  row class    labels of (H, k, G): how the image rows fall on the DMA groups (row_classes)
  grid class   labels of (N, geometry, nparts): how dw_finish rounds the grid and how workgroups walk the items (grid_classes)

CASES is the table: the smallest (W, C) found by a greedy cover of the reachable triples, H and N chosen for the row and grid
classes, and per case the `nparts` values its launches run with.  No GPU at import: everything here is host arithmetic, CPU tensors
and a plain fp32 emulation of the sweeps (emulate) that tests/test_dw_geometry_cpu.py uses to show that the checks of
tests/test_gpu_dw_geometry.py reject the fault each guard is there against."""
import ctypes as C
from collections import namedtuple

import torch
import torch.nn.functional as F

from mnasnet_pytorch_amd import _lib as L

FEATURES = (
    "more than one channel block",                       # cblocks > 1: dw_item's channel-block walk, cb0 of the tables
    "ragged last channel block (C/2 % cpw != 0)",        # ch_ok, (c0 + cgl*8) < C in dw_dma_plan, c < C in the table writes
    "idle lanes (sx*cpw < threads)",                     # active = sxi < sx
    "a wave copies two DMA blocks (nb > threads/64)",    # b = wave + nwaves in dw_dma_plan / dw_dma_rows / dw_fill_edges
    "ragged last DMA block (rc % 64 != 0)",              # q < rc
    "more than one strip per row",                       # x0 > 0: the left halo is image data, not fill
    "ragged last strip (W % (4*sx) != 0)",               # gx0 + ox < W on whole threads, gx < W in dw_dma_plan
    "W % 4 != 0",                                        # gx0 + ox < W inside a thread's four columns
)
WHICH = ("fwd", "bwd0", "bwd1", "bwd2")
Geo = namedtuple("Geo", "k which G cpw sx threads strips cblocks iw cgn rc nb nwaves feats")


def geometry(W, C_, k, which, N=2, H=7):
    """Geo of the launch form `which` at (W, C), or None where the library refuses the shape"""
    out = (C.c_int * 7)()
    if L.load().mnas_dw_geometry(N, H, W, C_, k, which, out) != 0:
        return None
    cpw, sx, threads, strips, cblocks, _, G = tuple(out)
    iw = 4 * sx + k - 1
    cgn = cpw // 4
    rc = iw * cgn
    nb = (rc + 63) // 64
    nwaves = threads // 64
    feats = (cblocks > 1, (C_ // 2) % cpw != 0, sx * cpw < threads, nb > nwaves, rc % 64 != 0, strips > 1, W % (4 * sx) != 0, W % 4 != 0)
    return Geo(k, which, G, cpw, sx, threads, strips, cblocks, iw, cgn, rc, nb, nwaves, feats)


def form_of(geo):
    return (geo.k, geo.which, geo.G)


def triples(geo):
    return {(form_of(geo), i, bool(v)) for i, v in enumerate(geo.feats)}


def second_block_live(geo, W):
    """whether a wave's second DMA block holds image data in some strip.  "A wave copies two DMA blocks" alone can be vacuous: on a
    1-column image the blocks past the first nwaves hold nothing but the right-hand padding columns, and a kernel that never copied
    them would compute the same (the fault injection of tests/test_dw_geometry_cpu.py found this on the first table).  Every form
    that can copy a second block therefore also needs a case where that block matters (EXTRA)."""
    pad, tw = geo.k // 2, 4 * geo.sx
    return any(0 <= s * tw - pad + q // geo.cgn < W for s in range(geo.strips) for q in range(64 * geo.nwaves, geo.rc))


EXTRA = "the second DMA block holds image columns"


def extras(geo, W):
    return {(form_of(geo), EXTRA)} if second_block_live(geo, W) else set()


# (form, feature index, value) that no (W, C) reaches, each with its arithmetic.  The 2-row search sees every candidate of the 4-row
# search with the same score, so 0.93 * score wins only where the best strip is one that 8-row rings cannot hold.  Phase 1 (two
# rings): 2 * 8 * iw * cpw * 4 B > 78 KB, i.e. iw * cpw > 1248 with sx * cpw <= 256 -- wide, channel-rich strips.
UNREACHABLE = [
    (((3, 2, 2), 3, False), "G = 2 needs iw*cpw > 1248, i.e. rc = iw*cpw/4 > 312 chunks = 5 DMA blocks, on at most 4 waves"),
    (((5, 2, 2), 3, False), "G = 2 needs iw*cpw > 1248, i.e. rc = iw*cpw/4 > 312 chunks = 5 DMA blocks, on at most 4 waves"),
    (((3, 2, 2), 2, True), "iw*cpw = (4*sx + 2)*cpw > 1248 with sx*cpw <= 256 needs cpw > 112, i.e. cpw in {116, 120, 124, 128} with "
                           "sx = 2; over the whole sweep only cpw = 128 ever wins the score (the CPU test asserts it): 256 lanes busy"),
    (((3, 2, 2), 4, True), "the only geometry is cpw = 128, sx = 2: rc = 10 * 32 = 320 = 5 * 64"),
]


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def row_classes(H, k, G):
    """labels of how H image rows fall on the sweep's DMA groups: groups of G rows start at row -PAD (PAD = k // 2), the sweep takes
    nsteps = ceil((H + 2 PAD) / G) steps, and the forward's read-ahead touches rows iy + 1, iy + 2 past the image"""
    pad = k // 2
    out = {"H % G == 0" if H % G == 0 else "H % G != 0"}
    if H == 1:
        out.add("H = 1")
    elif H <= pad:
        out.add("1 < H <= PAD")
    if H + 2 * pad <= G:
        out.add("single step")
    out.add("last row opens its group" if (H - 1 + pad) % G == 0 else "last row inside its group")
    return frozenset(out)


def reachable_row_classes(k, G):
    out = set()
    for H in range(1, 40):
        out |= row_classes(H, k, G)
    return frozenset(out)


# ---- grid ---------------------------------------------------------------------------------------------------------------------------
GRID_CLASSES = ("geff = cblocks", "geff < 8", "geff % 8 != 0", "geff = items", "items % geff != 0", "walks >= 3 items across images",
                "nparts % cblocks != 0", "nparts < cblocks")


def xcd_remap(b, n):
    """csrc/mnas_common.h: hardware workgroup b of n -> logical workgroup (consecutive logical ids share an XCD)"""
    q, r = n >> 3, n & 7
    xcd, slot = b & 7, b >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot


def grid(geo, N, nparts):
    """(geff, items) of dw_finish, geff = 0 where the launch returns MNAS_EINVAL"""
    items = N * geo.strips * geo.cblocks
    if nparts < geo.cblocks:
        return 0, items
    return min(nparts, items) // geo.cblocks * geo.cblocks, items


def grid_classes(geo, N, nparts):
    geff, items = grid(geo, N, nparts)
    if geff == 0:
        return frozenset({"nparts < cblocks"})
    out = set()
    if geff == geo.cblocks:
        out.add("geff = cblocks")
    if geff < 8:
        out.add("geff < 8")
    if geff % 8:
        out.add("geff % 8 != 0")
    if geff == items:
        out.add("geff = items")
    if items % geff:
        out.add("items % geff != 0")
    per_image = geo.strips * geo.cblocks
    for bid in range(geff):
        walk = range(bid, items, geff)
        if len(walk) >= 3 and walk[0] // per_image != walk[-1] // per_image:
            out.add("walks >= 3 items across images")
            break
    if nparts % geo.cblocks:
        out.add("nparts % cblocks != 0")
    return frozenset(out)


def item_of(geo, item):
    """dw_item: channel block fastest, then strip, then image -> (n, strip, channel block)"""
    cb = item % geo.cblocks
    r = item // geo.cblocks
    return r // geo.strips, r % geo.strips, cb


def column_items(geo, N, nparts):
    """{(table column r, channel block cb): [items]}: logical workgroup bid = r * cblocks + cb walks item = bid, bid + geff, ...
    (what xcd_remap must preserve: it permutes the hardware ids onto the logical ones, nothing else)"""
    geff, items = grid(geo, N, nparts)
    return {(bid // geo.cblocks, bid % geo.cblocks): list(range(bid, items, geff)) for bid in range(geff)}


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# (N, H, W, C, k, which, nparts): one launch form at one geometry.  nparts: the grids the case runs with -- the first is the one the
# dense references are checked on, the others carry grid classes and the "results do not depend on the grid" comparison; a value
# below the channel-block count comes last and must be refused.  (W, C): greedy cover of the reachable triples, smallest W*C first,
# pruned until every case is the only witness of something (tests/test_dw_geometry_cpu.py asserts both); H and nparts chosen for the
# row and grid classes.
Case = namedtuple("Case", "N H W C k which nparts")
CASES = [Case(*c) for c in (
    (3, 1, 1, 504, 3, 0, (3, 4, 6, 1)),
    (3, 8, 4, 128, 3, 0, (37, 1)),
    (3, 7, 17, 136, 3, 0, (37, 1)),
    (3, 1, 1, 504, 3, 1, (3, 4, 6, 1)),
    (3, 7, 4, 128, 3, 1, (37, 1)),
    (3, 7, 49, 40, 3, 1, (37, 1)),
    (3, 1, 8, 256, 3, 1, (37, 1)),
    (3, 7, 5, 424, 3, 1, (3, 37, 1)),
    (3, 7, 17, 136, 3, 1, (1, 5, 7)),
    (3, 8, 1, 504, 3, 2, (3, 4, 6, 1)),
    (3, 7, 4, 128, 3, 2, (37, 1)),
    (3, 6, 8, 256, 3, 2, (37, 1)),
    (3, 7, 17, 136, 3, 2, (37, 1)),
    (3, 7, 5, 504, 3, 2, (3, 37, 1)),
    (2, 7, 37, 256, 3, 2, (1, 3, 12)),
    (3, 7, 1, 504, 3, 3, (3, 4, 6, 1)),
    (3, 7, 4, 128, 3, 3, (37, 1)),
    (3, 7, 49, 40, 3, 3, (37, 1)),
    (3, 7, 8, 256, 3, 3, (37, 1)),
    (3, 7, 5, 424, 3, 3, (3, 37, 1)),
    (3, 7, 17, 136, 3, 3, (1, 5, 7)),
    (3, 2, 1, 8, 5, 0, (37, 1)),
    (3, 7, 1, 504, 5, 0, (3, 4, 6, 1)),
    (3, 8, 4, 128, 5, 0, (37, 1)),
    (3, 1, 17, 136, 5, 0, (37, 1)),
    (3, 2, 1, 504, 5, 1, (3, 4, 6, 1)),
    (3, 8, 4, 128, 5, 1, (37, 1)),
    (3, 7, 9, 88, 5, 1, (37, 1)),
    (3, 7, 49, 40, 5, 1, (37, 1)),
    (3, 7, 8, 256, 5, 1, (37, 2)),
    (3, 7, 5, 424, 5, 1, (8, 14, 21, 5)),
    (3, 7, 17, 136, 5, 1, (37, 1)),
    (3, 2, 1, 8, 5, 2, (37, 1)),
    (3, 7, 1, 504, 5, 2, (3, 4, 6, 1)),
    (3, 1, 4, 128, 5, 2, (37, 1)),
    (3, 7, 8, 256, 5, 2, (37, 1)),
    (3, 7, 5, 424, 5, 2, (3, 37, 1)),
    (3, 7, 17, 136, 5, 2, (37, 1)),
    (2, 7, 37, 256, 5, 2, (1, 3, 12)),
    (3, 1, 1, 504, 5, 3, (3, 4, 6, 1)),
    (3, 7, 4, 128, 5, 3, (37, 1)),
    (3, 7, 9, 88, 5, 3, (37, 1)),
    (3, 7, 49, 40, 5, 3, (37, 1)),
    (3, 7, 8, 256, 5, 3, (37, 2)),
    (3, 7, 5, 424, 5, 3, (8, 14, 21, 5)),
    (3, 7, 17, 136, 5, 3, (37, 1)),
)]


def case_id(c):
    return "k%d_%s_%dx%dx%dx%d" % (c.k, WHICH[c.which], c.N, c.H, c.W, c.C)


def case_geo(c):
    return geometry(c.W, c.C, c.k, c.which, c.N, c.H)


def case_grids(c):
    """(valid nparts values, refused ones)"""
    geo = case_geo(c)
    return [n for n in c.nparts if n >= geo.cblocks], [n for n in c.nparts if n < geo.cblocks]


def case_covers(c):
    """what the case reaches: its triples, (k, G, forward?, row class), (form, grid class) and (form, EXTRA)"""
    geo = case_geo(c)
    f = form_of(geo)
    rows = {(c.k, geo.G, c.which == 0, lab) for lab in row_classes(c.H, c.k, geo.G)}
    grids = {(f, lab) for n in c.nparts for lab in grid_classes(geo, c.N, n)}
    return triples(geo), rows, grids, extras(geo, c.W)


# ---- operands: built on the CPU from the case's own seed, so that the CPU test sees the very tensors the GPU test uploads -----------
def _u(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def _bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def ident_bn(C_):
    """bnbuf rows under which s*y+t = y, dy = g and xhat = y exactly (as test_gpu_kernels._ident_bn)"""
    b = torch.zeros(8, C_)
    b[0] = b[2] = b[6] = 1.0
    return b


def dense_operands(c):
    """fp32 CPU tensors holding bf16 values, drawn as test_gpu_bwd_forms._DwCase draws them: x (the forward's input, the weight
    gradient's activation and the fused reduce's mask input: off the hinge of bx), g and y (dy's operands, y off the hinge of b).
    The smallest cases hold under a hundred elements, where two elements on a bf16 rounding boundary already exceed the helpers'
    shares: the draw is repeated from the next seed until the conditions hold as the helpers state them (never more than a few times;
    tests/test_dw_geometry_cpu.py asserts them on the result)."""
    from bounds_conv import act_interval, dy_interval, off_hinge
    C_, k, shape = c.C, c.k, (c.N, c.H, c.W, c.C)
    for attempt in range(8):
        gen = torch.Generator().manual_seed(4100 + CASES.index(c) + 1000 * attempt)
        bx, b = torch.zeros(8, C_), torch.zeros(8, C_)
        bx[0], bx[1] = 1 + 0.3 * _u(gen, C_), 0.2 * _u(gen, C_)
        bx[5], bx[6] = 0.1 * _u(gen, C_), 1 + 0.2 * _u(gen, C_).abs()
        b[0], b[1] = 1 + 0.3 * _u(gen, C_), 0.2 * _u(gen, C_)
        b[2], b[3], b[4] = b[0], 0.05 * _u(gen, C_), 0.02 * _u(gen, C_)
        x, g, y = (_bf16r(_u(gen, *shape)) for _ in range(3))
        w, bias = _u(gen, C_, k, k) * (1.0 / k), 0.1 * _u(gen, C_)
        try:
            # (the materialised-input launches read the same x with scale = NULL and run without the fused reduce: no second hinge)
            x, y = off_hinge(x, bx[0], bx[1]), off_hinge(y, b[0], b[1])
            act_interval(x, bx[0], bx[1], True)
            dy_interval(g, y, b, True)
        except AssertionError:
            continue
        return dict(x=x, g=g, y=y, bx=bx, b=b, w=w, bias=bias, bi=ident_bn(C_))
    raise AssertionError("no draw of %s meets the operand conditions" % (c,))


def probe_pixels(c, geo):
    """flat live-pixel indices of the sparse probe (generalises test_gpu_kernels._dw_probe_case): the image corners of the first and
    last image; both sides of EVERY strip boundary on both sides of the first DMA row-group boundary inside the image (row 0 where
    there is none); columns W - 1 and 4*(W // 4) - 1 there and in the last row; the last row's middle"""
    N, H, W = c.N, c.H, c.W
    tw = 4 * geo.sx
    rb = next((r for r in range(geo.G - c.k // 2, H, geo.G) if r >= 1), None)
    rows = (0,) if rb is None else (rb - 1, rb)
    at = lambda n, h, w_: (n * H + h) * W + w_
    px = {at(n, h, w_) for n in (0, N - 1) for h in (0, H - 1) for w_ in (0, W - 1)}
    px |= {at(0, h, w_) for h in rows for s in range(1, geo.strips) for w_ in (s * tw - 1, s * tw)}
    edge = {W - 1} | ({4 * (W // 4) - 1} if W >= 4 else set())
    px |= {at(n, h, w_) for n in (0, N - 1) for h in rows + (H - 1,) for w_ in edge}
    px.add(at(N - 1, H - 1, W // 2))
    return sorted(px)


def sparse_operands(c, geo):
    """forward: a plain x live at probe_pixels (every channel), no bias.  Backward: g live there, y = 1 and the identity
    coefficients (dy = g exactly), x dense and read through the identity (act = relu(x) exactly)"""
    from bounds_conv import off_hinge
    gen = torch.Generator().manual_seed(5200 + CASES.index(c))
    px = probe_pixels(c, geo)
    shape = (c.N, c.H, c.W, c.C)
    live = torch.zeros(c.N * c.H * c.W, c.C)
    v = _bf16r(_u(gen, len(px), c.C))
    live[px] = torch.where(v.abs() < 0.25, torch.copysign(torch.full_like(v, 0.25), v) + v, v)       # (no live value near zero)
    live = _bf16r(live).view(shape)
    bi = ident_bn(c.C)
    w = _u(gen, c.C, c.k, c.k) * (1.0 / c.k)
    w = torch.where(w.abs() < 0.05, torch.full_like(w, 0.05), w)                                      # (no tap near zero)
    o = dict(px=px, w=w, bx=bi, b=bi, bi=bi, bias=None)
    if c.which == 0:
        o["x"] = live
    else:
        x = _bf16r(_u(gen, *shape))
        x = torch.where(x.abs() < 0.25, x.abs() + 0.25, x)            # (act = relu(x): away from the hinge, half of it live)
        o.update(x=off_hinge(_bf16r(x), bi[0], bi[1]), g=live, y=torch.ones(shape))
    return o


# ---- a plain fp32 emulation of the sweeps, item by item, with the fault of each guard ----------------------------------------------
FAULTS = ("strip_drop", "strip_dup", "ctail_drop", "dma2_zero", "rowgroup_drop", "oob_nonzero", "item_skip", "col_swap")


def fault_applies(fault, c, geo, nparts):
    geff, items = grid(geo, c.N, nparts)
    return {"strip_drop": geo.feats[6] or geo.feats[7], "strip_dup": geo.feats[6] or geo.feats[7], "ctail_drop": geo.feats[1],
            "dma2_zero": second_block_live(geo, c.W), "rowgroup_drop": True, "oob_nonzero": c.which != 2, "item_skip": items > geff,
            "col_swap": geff // geo.cblocks >= 2}[fault]


def emulate(c, geo, o, nparts, virt=True, red=True, masked=False, fault=None):
    """One launch of form c.which as csrc/mnas_dw.hip describes it, in fp32 on the CPU: workgroup bid of geff walks the items
    bid, bid + geff, ...; an item is one image, one strip of 4*sx columns and one channel block; its ring window holds iw columns from
    x0 - PAD, in 16-byte chunks q = column * cgn + channel group, blocks of 64 chunks; outputs and sums come from the strip's own
    columns; every workgroup writes column bid // cblocks of the partial tables.  Unwritten outputs stay NaN (the guarded buffers'
    "never written").  fault: one of FAULTS -- what the kernel would do if the guard named in FEATURES were wrong."""
    N, H, W, C_, k, which = c[:6]
    pad, G, tw, iw, cblk = k // 2, geo.G, 4 * geo.sx, geo.iw, 2 * geo.cpw
    geff, items = grid(geo, N, nparts)
    assert geff > 0
    rows = geff // geo.cblocks
    fwd, DG, WG = which == 0, which in (1, 2), which in (1, 3)
    RED = red and DG
    bx, b = o["bx"], o["b"]
    rbn = bx if virt else o["bi"]                  # the bnbuf of the producer of x: a materialised x is read through the identity
    xs, xt = rbn[0], rbn[1]
    nsteps = (H + 2 * pad + G - 1) // G
    row_cut = (nsteps - 1) * G - 2 * pad if fault == "rowgroup_drop" else H          # output rows from row_cut on are never emitted
    res = dict(rows=rows)
    outp = torch.full((N, H, W, C_), float("nan"))
    stats = torch.full((2, C_, rows), float("nan"))
    wpart = torch.full((rows, k * k, C_), float("nan"))
    redp = torch.full((2, C_, rows), float("nan"))
    chunk = torch.arange(iw).view(-1, 1) * geo.cgn
    for bid in range(geff):
        col, cb = bid // geo.cblocks, bid % geo.cblocks
        c0 = cb * cblk
        c1 = min(c0 + cblk, C_)
        if fault == "ctail_drop" and cb == geo.cblocks - 1:
            c1 -= 8
        ch = slice(c0, c1)
        nch = c1 - c0
        second = (chunk + (torch.arange(nch) // 8).view(1, -1)) >= 64 * geo.nwaves          # chunks of a wave's second DMA block
        s1, s2 = torch.zeros(nch), torch.zeros(nch)
        wacc = torch.zeros(k * k, nch)
        walk = list(range(bid, items, geff))
        if fault == "item_skip" and bid == 0:
            del walk[1:2]
        for item in walk:
            n, strip, _ = item_of(geo, item)
            x0 = strip * tw
            cols = torch.arange(x0 - pad, x0 - pad + iw)
            inimg = (cols >= 0) & (cols < W)
            ocol = x0 + torch.arange(tw)
            valid = ocol < W
            last4 = valid & (ocol >= 4 * ((W - 1) // 4)) & (strip == geo.strips - 1)
            if fault == "strip_drop":
                valid = valid & ~last4
            wsum = valid.float() + (last4.float() if fault == "strip_dup" else 0.0)          # weight of a column in the sums
            wsum = wsum.view(1, -1, 1)

            def ring(src):
                win = torch.zeros(H, iw, nch)
                win[:, inimg] = src[n][:, cols[inimg], ch]
                if fault == "dma2_zero":
                    win[:, second] = 0.0
                return win

            def act_window():
                raw = ring(o["x"])
                if fault == "oob_nonzero":
                    raw[:, ~inimg] = 1.0
                a = torch.relu(xs[ch] * raw + xt[ch]) if virt else raw
                if fault != "oob_nonzero":
                    a[:, ~inimg] = 0.0
                return a

            def conv(win, wt, bias=None):          # [H, iw, nch] -> [H, tw, nch]: k x k taps, rows zero-padded, columns from the window
                r = F.conv2d(win.permute(2, 0, 1).unsqueeze(0), wt.reshape(nch, 1, k, k), bias, padding=(pad, 0), groups=nch)
                return r[0].permute(1, 2, 0)

            emit = torch.zeros(H, tw, dtype=torch.bool)
            emit[:row_cut] = True
            emit &= valid.view(1, -1)
            if fwd:
                v = conv(act_window(), o["w"][ch], None if o["bias"] is None else o["bias"][ch])
                vs = v * (wsum * (torch.arange(H) < row_cut).view(-1, 1, 1))
                s1 += vs.sum((0, 1))
                s2 += (vs * v).sum((0, 1))
                stored = _bf16r(v)
            else:
                gr, yr = ring(o["g"]), ring(o["y"])
                dz = gr if masked else torch.where(b[0][ch] * yr + b[1][ch] > 0, gr, torch.zeros_like(gr))
                dy = b[2][ch] * dz + (b[3][ch] * yr + b[4][ch])
                dy[:, ~inimg] = 0.0
                if DG:
                    stored = _bf16r(conv(dy, o["w"][ch].flip(-1, -2)))
                if WG:
                    ap = torch.zeros(H + 2 * pad, iw, nch)
                    ap[pad:pad + H] = act_window()
                    dyc = dy[:, pad:pad + tw] * (wsum * (torch.arange(H) < row_cut).view(-1, 1, 1))
                    for ky in range(k):
                        for kx in range(k):
                            wacc[ky * k + kx] += (dyc * ap[ky:ky + H, kx:kx + tw]).sum((0, 1))
                if RED:
                    xraw = ring(o["x"])[:, pad:pad + tw]
                    dzr = torch.where(xs[ch] * xraw + xt[ch] > 0, stored, torch.zeros_like(stored))
                    dzr = dzr * (wsum * (torch.arange(H) < row_cut).view(-1, 1, 1))
                    s1 += dzr.sum((0, 1))
                    s2 += (dzr * (xraw * rbn[6][ch] - rbn[5][ch] * rbn[6][ch])).sum((0, 1))
            if fwd or DG:
                dst = outp[n, :, x0:x0 + tw, ch]
                m = emit[:, :dst.shape[1]].unsqueeze(-1).expand_as(dst)
                dst[m] = stored[:, :dst.shape[1]][m]
        stats[:, ch, col] = torch.stack((s1, s2))
        redp[:, ch, col] = torch.stack((s1, s2))
        wpart[col, :, ch] = wacc
    if fault == "col_swap":
        for t in (stats, redp):
            t[:, :, [0, 1]] = t[:, :, [1, 0]]
        wpart[[0, 1]] = wpart[[1, 0]]
    if fwd:
        res.update(out=outp, stats=stats)
    else:
        res.update(gin=outp if DG else None, wpart=wpart if WG else None, red=redp if RED else None)
    return res


# ---- references and checks, shared by the emulation (CPU) and the launches (GPU) ---------------------------------------------------
def _by_column(geo, N, nparts, q):
    """q [..., N, W, C] of per-pixel-column fp64 sums -> [..., rows, C]: column r of channel block cb holds the sum over exactly the
    items that item = r*cblocks + cb (mod geff) assigns to it (dw_item: channel block fastest, then strip, then image)"""
    geff, _ = grid(geo, N, nparts)
    tw, cblk = 4 * geo.sx, 2 * geo.cpw
    out = torch.zeros(q.shape[:-3] + (geff // geo.cblocks, q.shape[-1]), dtype=torch.float64, device=q.device)
    for (r, cb), its in column_items(geo, N, nparts).items():
        ch = slice(cb * cblk, (cb + 1) * cblk)
        for it in its:
            n, strip, _ = item_of(geo, it)
            out[..., r, ch] += q[..., n, strip * tw:(strip + 1) * tw, ch].sum(-2)
    return out


class Refs:
    """fp64 references of one case's operands on `device`, each computed once and left unchanged"""

    def __init__(self, c, geo, o, device, exact=False):
        """exact: the sparse probe's operands -- read through the identity, act = relu(x) and dy = g with no rounding at all"""
        self.c, self.geo, self.o, self.dev, self.exact, self._memo = c, geo, o, device, exact, {}

    def _get(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def act(self, virt):
        from bounds_conv import act_interval
        from intervals import Interval
        o = self.o
        if self.exact:
            return self._get(("act", virt), lambda: Interval.exact(torch.relu(o["x"]) if virt else o["x"], self.dev))
        return self._get(("act", virt), lambda: act_interval(o["x"], o["bx"][0], o["bx"][1], False, self.dev) if virt
                         else Interval.exact(o["x"], self.dev))

    def dy(self):
        from bounds_conv import dy_interval
        from intervals import Interval
        o = self.o
        if self.exact:
            return self._get("dy", lambda: Interval.exact(o["g"], self.dev))
        return self._get("dy", lambda: dy_interval(o["g"], o["y"], o["b"], False, self.dev))

    def fwd(self, virt, bias):
        from bounds_conv import dw_fwd_terms
        return self._get(("fwd", virt, bias), lambda: dw_fwd_terms(self.act(virt), self.o["w"], self.o["bias"] if bias else None, 1, self.dev))

    def gin(self):
        from bounds_conv import dw_dgrad_terms
        return self._get("gin", lambda: dw_dgrad_terms(self.dy(), self.o["w"], self.c.H, self.c.W, 1, self.dev))

    def wgrad_cols(self, virt):
        """(ref, S, slack) of the weight gradient per pixel column of dy: [N, W, C, k, k] each (their sum over N, W is dw_wgrad_terms)"""
        def make():
            from refs64 import pad_hw
            a, d, k, H, W = self.act(virt), self.dy(), self.c.k, self.c.H, self.c.W
            out = []
            for xa, da in ((a.mid, d.mid), (a.amax, d.amax), (a.mid.abs(), d.mid.abs())):
                xp = pad_hw(xa, k // 2)
                t = torch.zeros(xa.shape[0], W, xa.shape[3], k, k, dtype=torch.float64, device=self.dev)
                for kh in range(k):
                    for kw in range(k):
                        t[..., kh, kw] = (xp[:, kh:kh + H, kw:kw + W] * da).sum(1)
                out.append(t)
            return out[0], out[1], (out[1] - out[2]).clamp_min(0)
        return self._get(("wg", virt), make)


def _family(c, what):
    return "dw geometry %s: %s" % (WHICH[c.which], what)


def check_table(c, geo, nparts, hip, terms, cc, what, family):
    """Per-column check of a partial table.  hip [rows, C]; terms (ref, S, slack) [N, W, C] per pixel column: every column within
    check_sum_bound's bound (M = all pixels, one slab) of the fp64 sum over its own items"""
    from intervals import check_sum_bound
    ref, S, slack = (_by_column(geo, c.N, nparts, t) for t in terms)
    assert hip.shape == ref.shape, (what, hip.shape, ref.shape)
    return check_sum_bound(hip.to(ref.device), ref, S, c.N * c.H * c.W, 1, cc, what + " by table column", slack, family)


def check_fwd(c, geo, refs, res, nparts, virt, bias, what, dense=True):
    from bounds_conv import check_dw_bound, check_stats_bound, dw_elem_err, stats_bound_terms
    fam = "" if dense else "sparse "
    r64, S = refs.fwd(virt, bias)
    check_dw_bound(res["out"].to(r64.device), r64, S, c.k, what + " out", _family(c, fam + "output"))
    st = res.get("stats")
    if st is None:
        return
    e = dw_elem_err(S, c.k)
    check_stats_bound(st.to(r64.device), r64, e, c.N * c.H * c.W, what, _family(c, fam + "statistics"))
    t = stats_bound_terms(r64, e, dims=(1,))                          # per (image, pixel column, channel)
    check_table(c, geo, nparts, st[0].t(), (t[0], t[1], t[2]), 1, what + " stats sum", _family(c, fam + "table columns"))
    check_table(c, geo, nparts, st[1].t(), (t[3], t[4], t[5]), 2, what + " stats sum of squares", _family(c, fam + "table columns"))


def check_bwd(c, geo, refs, res, nparts, virt, grad, what, dense=True):
    """grad: the finalized weight gradient [C, k, k] (mnas_dw_wgrad_finalize on the device, the fp64 sum of the rows for the emulation)"""
    from bounds_conv import check_dw_bound, check_red_bound, relu_mask
    from intervals import check_sum_bound
    fam = "" if dense else "sparse "
    o, dev = refs.o, refs.dev
    M = c.N * c.H * c.W
    gin = res.get("gin")
    if gin is not None:
        r64, S = refs.gin()
        gin = gin.to(dev)
        check_dw_bound(gin, r64, S, c.k, what + " gin", _family(c, fam + "input gradient"))
    if res.get("wpart") is not None:
        ref, S, slack = refs.wgrad_cols(virt)
        check_sum_bound(grad.to(dev), ref.sum((0, 1)), S.sum((0, 1)), M, res["rows"], 2, what + " dW", slack.sum((0, 1)),
                        _family(c, fam + "weight gradient"))
        kk = c.k * c.k
        flat = lambda t: t.reshape(t.shape[:3] + (kk,)).permute(3, 0, 1, 2)                # [k*k, N, W, C]
        tabs = [_by_column(geo, c.N, nparts, flat(t)).permute(1, 0, 2) for t in (ref, S, slack)]      # [rows, k*k, C]
        check_sum_bound(res["wpart"].to(dev), tabs[0], tabs[1], M, 1, 2, what + " wpartial by table row", tabs[2],
                        _family(c, fam + "table columns"))
    if res.get("red") is not None:
        bn = o["bx"] if virt else o["bi"]
        x = o["x"].to(dev)
        check_red_bound(res["red"].to(dev), gin.float(), x, bn, M, what, _family(c, fam + "fused reduce"))
        bn = bn.double().to(dev)
        dz = gin.double() * relu_mask(x, bn[0], bn[1])
        xhat, xabs = (x.double() - bn[5]) * bn[6], (x.double().abs() + bn[5].abs()) * bn[6].abs()
        for i, (r_, s_, cc) in enumerate(((dz, dz.abs(), 1), (dz * xhat, dz.abs() * xabs, 2))):
            check_table(c, geo, nparts, res["red"][i].t(), (r_.sum(1), s_.sum(1), torch.zeros_like(r_.sum(1))), cc,
                        what + " reduce %d" % i, _family(c, fam + "table columns"))


def check_sparse(c, geo, refs, res, grad, what):
    """the sparse probe's own conditions: outputs outside the k x k neighbourhood of every live pixel exactly zero (plain operands:
    the products are exact zeros), and each live pixel's own contribution to the weight gradient / the statistics sum above twice
    the bound (dropping or doubling it would leave the bound)"""
    from intervals import sum_bound
    o, dev, k, pad = refs.o, refs.dev, c.k, c.k // 2
    M, rows = c.N * c.H * c.W, res["rows"]
    live = torch.zeros(M, dtype=torch.bool)
    live[o["px"]] = True
    near = F.max_pool2d(live.view(c.N, 1, c.H, c.W).float(), k, 1, pad).view(c.N, c.H, c.W) > 0
    out = res.get("out") if c.which == 0 else res.get("gin")
    if out is not None:
        assert not bool(out.to("cpu")[~near].any()), "%s: an output away from every live pixel is not zero" % what
    if c.which == 0 and res.get("stats") is not None:
        r64, S = refs.fwd(False, False)
        from bounds_conv import dw_elem_err, stats_bound_terms
        _, S1, k1, _, _, _ = stats_bound_terms(r64, dw_elem_err(S, k))
        bound = sum_bound(S1, M, rows, 1, k1).cpu()
        inside = torch.zeros(c.N, c.H + 2 * pad, c.W + 2 * pad)
        inside[:, pad:pad + c.H, pad:pad + c.W] = 1.0
        for p in o["px"]:                                  # x pixel p reaches output (h - ky + pad, w - kx + pad) through tap (ky, kx)
            n, h, w_ = p // (c.H * c.W), p // c.W % c.H, p % c.W
            taps = inside[n, h:h + k, w_:w_ + k].flip(0, 1)
            contrib = o["x"].view(M, c.C)[p].double() * (o["w"].double() * taps).sum((1, 2))
            assert bool((contrib.abs() > 2 * bound).any()), "%s: the probe could not see pixel %d dropped from the statistics" % (what, p)
    if c.which in (1, 3):
        ref, S, slack = refs.wgrad_cols(True)
        assert float(slack.max()) == 0.0
        bound = sum_bound(S.sum((0, 1)), M, rows, 2).cpu()
        ap = torch.zeros(c.N, c.H + 2 * pad, c.W + 2 * pad, c.C, dtype=torch.float64)
        ap[:, pad:pad + c.H, pad:pad + c.W] = torch.relu(o["x"]).double()
        for p in o["px"]:
            n, h, w_ = p // (c.H * c.W), p // c.W % c.H, p % c.W
            contrib = ap[n, h:h + k, w_:w_ + k].permute(2, 0, 1) * o["g"].view(M, c.C)[p].double().view(-1, 1, 1)
            assert bool((contrib.abs() > 2 * bound).any()), "%s: the probe could not see pixel %d dropped from dW" % (what, p)
