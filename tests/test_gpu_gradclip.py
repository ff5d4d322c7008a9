"""-m gpu: global-norm gradient clipping, the non-finite skip and the weight EMA on the flat buffers (include/mnas.h:
mnas_grad_sqnorm, mnas_*_step_ex; train_step.FlatAdam / Trainer).  Oracles: tests/gradclip_ref.py (numpy, the arithmetic the header
specifies) and torch's own CPU optimizers fed the gradient the helper clipped."""
import ctypes

import numpy as np
import pytest
import torch

import cases as C
import gradclip_ref as R
from test_gpu_train import _no_dropout, build, rl2

pytestmark = pytest.mark.gpu

KINDS = [("rmsprop", {}), ("rmsprop", {"momentum": 0.9}), ("sgd", {}), ("sgd", {"momentum": 0.9}),
         ("sgd", {"momentum": 0.9, "nesterov": True}), ("adam", {})]          # test_flat_optimizers_match_torch's list
GUARD = 1e30
# mnas_grad_sqnorm: grid = min(256, ceil(n / 1024)) workgroups of 256 lanes, four elements per lane and loop trip
#   257: second grid-stride element of a lane; 1025: second workgroup; 262145 = 256 * 256 * 4 + 1: second loop trip of a lane
NORM_SIZES = [1, 255, 256, 257, 1025, 10007, 65537, 262145]


def _lib():
    from mnasnet_pytorch_amd import _lib as Lb
    return Lb, Lb.load()


def _guarded(values):
    """values at element offset 3 of a larger buffer whose other elements are 1e30 (an unaligned run between guards)"""
    n = values.numel()
    big = torch.full((n + 8,), GUARD, dtype=torch.float32, device="cuda")
    big[3:3 + n] = values.cuda()
    return big, big.data_ptr() + 12


def _sqnorm(ptr, n, scale, partial, off):
    Lb, lib = _lib()
    got = ctypes.c_int(-1)
    rc = lib.mnas_grad_sqnorm(ptr, n, scale, partial.data_ptr(), off, ctypes.byref(got), Lb.cur_stream())
    return rc, got.value


def _norm_coef(partial, nparts, max_norm=0.0):
    """(norm, coef) as the *_step_ex kernels derive them from the table: one launch over a 4-element dummy with lr = 0"""
    Lb, lib = _lib()
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    p, g = torch.ones(4, device="cuda"), torch.zeros(4, device="cuda")
    ex = Lb.MnasOptExtra(partial=partial.data_ptr(), nparts=nparts, max_norm=max_norm, skip_nonfinite=0, ema=None, ema_decay=0.0,
                         stats=stats.data_ptr(), update_stats=1)
    Lb.check(lib.mnas_sgd_step_ex(p.data_ptr(), g.data_ptr(), None, 4, 0.0, 0.0, 0.0, 0.0, 0, 1, 1.0, ctypes.byref(ex),
                                  Lb.cur_stream()))
    raw = Lb.MnasGradStats()
    host = stats.cpu()
    ctypes.memmove(ctypes.byref(raw), host.data_ptr(), 32)
    assert raw.steps == 1
    return np.float32(raw.last_norm), np.float32(raw.last_coef)


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_kernel(n, scale):
    """|norm_gpu - norm_ref| <= 2^-23 norm_ref: one fp32 rounding of the final value (the fp64 summation error is below 2^-40).
    The run starts at element 3 of a buffer and is surrounded by 1e30: a guard read into the sum would show at once."""
    gen = torch.Generator().manual_seed(1000 + n)
    vals = torch.randn(n, generator=gen) * 0.7
    big, ptr = _guarded(vals)
    partial = torch.full((1024,), -1.0, dtype=torch.float64, device="cuda")
    rc, nparts = _sqnorm(ptr, n, scale, partial, 0)
    assert rc == 0 and nparts == min(256, (n + 1023) // 1024)
    first = partial.cpu().clone()
    ref = R.norm(vals.numpy(), scale)
    # the table itself: slots beyond nparts untouched, the used ones sum to the helper's float64 sum
    assert bool((first[nparts:] == -1.0).all())
    s_ref = R.sqsum(vals.numpy(), scale)
    assert abs(float(first[:nparts].sum()) - s_ref) <= 2.0 ** -40 * s_ref
    got, coef = _norm_coef(partial, nparts, max_norm=0.25)
    print("n %d scale %g: norm gpu %.9g ref %.9g" % (n, scale, got, ref))
    assert abs(float(got) - float(ref)) <= 2.0 ** -23 * float(ref)
    c_ref = R.coef(ref, 0.25)
    assert abs(float(coef) - float(c_ref)) <= 2.0 ** -22 * float(c_ref)
    # two runs: bitwise equal tables
    partial.fill_(-1.0)
    assert _sqnorm(ptr, n, scale, partial, 0) == (0, nparts)
    assert torch.equal(partial.cpu(), first)
    assert bool((big[:3] == GUARD).all()) and bool((big[3 + n:] == GUARD).all())            # (the kernel only reads)


def test_norm_kernel_edge_values():
    partial = torch.zeros(1024, dtype=torch.float64, device="cuda")
    # all zero: norm 0, coef 1 (max_norm / 1e-6 clamps), nothing NaN
    big, ptr = _guarded(torch.zeros(5000))
    rc, k = _sqnorm(ptr, 5000, 1.0, partial, 0)
    assert rc == 0 and k == 5
    norm, coef = _norm_coef(partial, k, max_norm=1.0)
    assert norm == 0 and coef == 1
    # 1e25 in every element: the fp32 square would overflow, the fp64 one does not
    vals = torch.full((5000,), 1e25)
    big, ptr = _guarded(vals)
    assert _sqnorm(ptr, 5000, 1.0, partial, 0) == (0, 5)
    norm, coef = _norm_coef(partial, 5, max_norm=1.0)
    ref = R.norm(vals.numpy())
    assert np.isfinite(norm) and abs(float(norm) - float(ref)) <= 2.0 ** -23 * float(ref)
    assert abs(float(coef) - float(R.coef(ref, 1.0))) <= 2.0 ** -22 * float(R.coef(ref, 1.0))


def test_norm_two_runs_one_table_and_capacity():
    gen = torch.Generator().manual_seed(5)
    a, b = torch.randn(3001, generator=gen), torch.randn(1500, generator=gen) * 2.0
    (ba, pa), (bb, pb) = _guarded(a), _guarded(b)
    partial = torch.full((1024,), -1.0, dtype=torch.float64, device="cuda")
    rc, ka = _sqnorm(pa, 3001, 0.5, partial, 0)
    assert (rc, ka) == (0, 3)
    rc, kb = _sqnorm(pb, 1500, 0.5, partial, ka)
    assert (rc, kb) == (0, 2)
    norm, _ = _norm_coef(partial, ka + kb)
    ref = R.norm([a.numpy(), b.numpy()], 0.5)
    assert abs(float(norm) - float(ref)) <= 2.0 ** -23 * float(ref)
    # past the capacity: MNAS_EINVAL and nothing launched (the table is untouched)
    Lb, _ = _lib()
    before = partial.cpu().clone()
    rc, k = _sqnorm(pa, 3001, 0.5, partial, 1022)
    assert rc == Lb.EINVAL and k == -1
    rc, k = _sqnorm(pa, 3001, 0.5, partial, 1021)               # 1021 + 3 = 1024: the last slots
    assert (rc, k) == (0, 3)
    after = partial.cpu()
    assert torch.equal(after[:1021], before[:1021]) and torch.equal(after[1021:], before[:3])


def _flat_pair(kind, kw, p0, **extras):
    from mnasnet_pytorch_amd.train_step import FlatAdam, FlatRMSprop, FlatSGD
    n = p0.numel()
    flat_p, flat_g = p0.clone().cuda(), torch.zeros(n, device="cuda")
    par = torch.nn.Parameter(flat_p.view(n))
    par.data = flat_p.view(n)
    fcls = {"adam": FlatAdam, "rmsprop": FlatRMSprop, "sgd": FlatSGD}[kind]
    return fcls([par], flat_p, flat_g, lr=1e-2, weight_decay=1e-2, **kw, **extras), flat_p, flat_g


def _torch_ref(kind, kw, p0):
    ref = torch.nn.Parameter(p0.clone())
    cls = {"adam": torch.optim.Adam, "rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}[kind]
    return ref, cls([ref], lr=1e-2, weight_decay=1e-2, **kw)


def _grads(n=10007, steps=5):
    g0 = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=g0)
    return p0, [torch.randn(n, generator=g0) * (0.5 + 0.2 * i) for i in range(steps)]


@pytest.mark.parametrize("kind,kw", KINDS)
def test_clipped_optimizers_match_torch(kind, kw):
    """test_flat_optimizers_match_torch's setting with grad_scale 0.5 and clip_grad_norm 50: the scaled gradients' norms are about
    25, 35, 45, 55, 65, so two of the five steps clip.  torch's optimizer on CPU gets the helper's (g * 0.5) * coef."""
    p0, grads = _grads()
    ref, opt_ref = _torch_ref(kind, kw, p0)
    opt, flat_p, flat_g = _flat_pair(kind, kw, p0, clip_grad_norm=50.0)
    opt.grad_scale = 0.5
    coefs = []
    for g in grads:
        nrm, c, gc = R.clipped(g.numpy(), 50.0, 0.5)
        coefs.append(c)
        ref.grad = torch.from_numpy(gc).clone()
        opt_ref.step()
        flat_g.copy_(g.cuda())
        opt.step()
    st = opt.grad_stats()
    print(kind, kw, "coefs", [float(c) for c in coefs], st)
    assert [bool(c < 1) for c in coefs] == [False, False, False, True, True]
    assert rl2(flat_p.cpu(), ref.detach()) < 1e-6, (kind, kw)
    assert st.steps == 5 and st.clipped_steps == 2 and st.skipped_steps == 0
    assert abs(st.last_coef - float(coefs[-1])) <= 2.0 ** -22 * float(coefs[-1])
    nrm_ref = float(R.norm(grads[-1].numpy(), 0.5))
    assert abs(st.last_norm - nrm_ref) <= 2.0 ** -23 * nrm_ref
    assert float(opt.last_grad_norm.cpu()[0]) == st.last_norm and opt.last_grad_norm.is_cuda


@pytest.mark.parametrize("kind,kw", KINDS)
def test_never_clipping_bound_is_a_noop(kind, kw):
    """coef == 1.0f: (g * gscale) * 1 is the plain kernels' gradient bit for bit"""
    p0, grads = _grads(steps=3)
    plain, p_a, g_a = _flat_pair(kind, kw, p0)
    ex, p_b, g_b = _flat_pair(kind, kw, p0, clip_grad_norm=1e30)
    for g in grads:
        g_a.copy_(g.cuda())
        g_b.copy_(g.cuda())
        plain.step()
        ex.step()
    assert torch.equal(p_a, p_b) and torch.equal(plain.flat_m, ex.flat_m) and torch.equal(plain.flat_v, ex.flat_v)
    st = ex.grad_stats()
    assert st.steps == 3 and st.clipped_steps == 0 and st.skipped_steps == 0 and st.last_coef == 1.0
    assert plain.grad_stats().steps == 0                              # the plain path moves no counters


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind,kw", [("adam", {}), ("rmsprop", {"momentum": 0.9}), ("sgd", {"momentum": 0.9})])
def test_skip_nonfinite(kind, kw, bad):
    """One NaN (then one +inf) in the gradient of step 2 of 3 -- a data value, the kernels just see a non-finite norm.  p, both
    moments and the EMA are bitwise unchanged across step 2, step 3 updates normally.  RMSprop and SGD keep no step count, so
    there the end state is torch's with step 2 left out (1e-6, the bound of the five-step test)."""
    p0, grads = _grads(steps=3)
    grads[1][4321] = bad
    opt, flat_p, flat_g = _flat_pair(kind, kw, p0, clip_grad_norm=60.0, skip_nonfinite=True, ema_decay=0.9)
    ref, opt_ref = _torch_ref(kind, kw, p0)
    for i, g in enumerate(grads):
        before = [t.clone() for t in (flat_p, opt.flat_m, opt.flat_v, opt.flat_ema)]
        flat_g.copy_(g.cuda())
        opt.step()
        same = [torch.equal(a, b) for a, b in zip(before, (flat_p, opt.flat_m, opt.flat_v, opt.flat_ema))]
        if i == 1:
            assert all(same), same
        else:
            assert not same[0] and not same[3] and bool(torch.isfinite(flat_p).all()) and bool(torch.isfinite(opt.flat_ema).all())
            ref.grad = torch.from_numpy(R.clipped(g.numpy(), 60.0)[2]).clone()
            opt_ref.step()
    st = opt.grad_stats()
    assert st.steps == 3 and st.skipped_steps == 1 and st.clipped_steps == (1 if float(R.norm(grads[2].numpy())) > 60.0 else 0)
    if kind != "adam":
        assert rl2(flat_p.cpu(), ref.detach()) < 1e-6
    # without the flag the non-finite norm propagates as in torch (error_if_nonfinite = False): a NaN norm makes every element NaN
    if bad != bad:
        opt2, p2, g2 = _flat_pair(kind, kw, p0, clip_grad_norm=60.0)
        g2.copy_(grads[1].cuda())
        opt2.step()
        assert bool(torch.isnan(p2).all()) and opt2.grad_stats().skipped_steps == 0


@pytest.mark.parametrize("d,clip", [(0.9, 40.0), (0.9999, None)])
def test_ema_per_element(d, clip):
    """Three parameters in one flat buffer, the middle one frozen: two trainable runs, [0, 1001) and [1038, 6041), both the frozen
    run and the second trainable one start off a 16-byte boundary.  After every step, per element:
    |ema_gpu - (d ema_prev + (1 - d) p_new)| <= 2^-23 (|d ema_prev| + |(1 - d) p_new|)  (two fp32 roundings); frozen elements of the
    shadow stay bitwise equal to p.  The frozen gradient is 1e30: it must stay out of the norm.  clip None: the EMA-only step (no
    norm launches)."""
    from mnasnet_pytorch_amd.train_step import FlatRMSprop
    sizes = [1001, 37, 5003]
    n = sum(sizes)
    gen = torch.Generator().manual_seed(3)
    flat_p, flat_g = torch.randn(n, generator=gen).cuda(), torch.zeros(n, device="cuda")
    params, off = [], 0
    for k in sizes:
        par = torch.nn.Parameter(flat_p[off:off + k])
        par.data = flat_p[off:off + k]
        params.append(par)
        off += k
    params[1].requires_grad_(False)
    opt = FlatRMSprop(params, flat_p, flat_g, lr=1e-2, momentum=0.9, clip_grad_norm=clip, ema_decay=d)
    assert opt._trainable_runs() == [[0, 1001], [1038, n]]
    p_start = flat_p.cpu().clone()
    frozen = slice(1001, 1038)
    for step in range(3):
        g = torch.randn(n, generator=gen) * (0.4 + 0.3 * step)
        g[frozen] = GUARD
        prev = opt.flat_ema.cpu().numpy().copy()
        flat_g.copy_(g.cuda())
        opt.step()
        p_new, ema = flat_p.cpu().numpy(), opt.flat_ema.cpu().numpy()
        want, bound = R.ema_bound(d, prev, p_new)
        err = np.abs(ema.astype(np.float64) - want)
        train = np.r_[0:1001, 1038:n]
        assert (err[train] <= bound[train]).all(), (step, float((err[train] / bound[train]).max()))
        assert np.array_equal(ema[frozen], p_new[frozen]) and np.array_equal(p_new[frozen], p_start.numpy()[frozen])
        assert not np.array_equal(ema[train], prev[train]) and not np.array_equal(ema[train], p_new[train])
        st = opt.grad_stats()
        assert st.steps == step + 1
        if clip is not None:
            ref = float(R.norm([g.numpy()[:1001], g.numpy()[1038:]]))
            assert abs(st.last_norm - ref) <= 2.0 ** -23 * ref and np.isfinite(st.last_norm)
            assert (st.last_coef < 1.0) == (ref > clip)
        else:
            assert st.last_norm == 0.0 and st.last_coef == 1.0 and opt._partial is None


@pytest.mark.parametrize("n", [1, 255, 257, 10007, 2048 * 256 + 300])
@pytest.mark.parametrize("kind", ["adam", "rmsprop", "sgd"])
def test_ex_kernels_per_element_bracket(kind, n):
    """ONE launch of mnas_<kind>_step_ex from a given state (bounds_tail.opt_case) with the fp64 partial table handed in directly
    (three values whose sum is exact in any order, so norm and coef are gradclip_ref's): clip active (coef < 1: gi takes one more
    rounding) and inactive, EMA off / decay 0 / decay 0.999, at element offsets 1 and 3 of guarded buffers; then a NaN and an
    Inf table under skip_nonfinite: every buffer bitwise untouched, steps and skipped_steps move."""
    import bounds_tail as BT
    assert BT.OPT_SIZES[-1] > BT.OPT_GRID_CAP == 2048 * 256 and n in BT.OPT_SIZES
    p, g, m, v, buf = BT.opt_data(n, seed=n + 1)
    st = dict(p=p, g=g, m=m, v=v, buf=buf, ema=p * 0.75 + 0.01)
    a = {"adam": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=2, gscale=0.125),
         "rmsprop": dict(lr=1e-2, alpha=0.99, eps=1e-8, wd=1e-2, momentum=0.9, gscale=1.0 / 3),
         "sgd": dict(lr=1e-2, momentum=0.9, dampening=0.5, wd=0.0, nesterov=0, step=2, gscale=0.125)}[kind]
    table = [2.25, 4.0, 0.0625]                        # norm = sqrt(6.3125)
    worst, k = 0.0, 0
    for max_norm in (0.9, 1e3):
        for ema, decay in ((False, 0.0), (True, 0.0), (True, 0.999)):
            ex = dict(partial=table, max_norm=max_norm, skip=1, ema=ema, decay=decay)
            worst, k = max(worst, BT.opt_case(kind, st, a, (1, 3)[k % 2], ex, family="optimizers, _ex")), k + 1
    for bad in (float("nan"), float("inf")):
        BT.opt_case(kind, st, a, 1, dict(partial=[2.25, bad, 0.0625], max_norm=0.9, skip=1, ema=True, decay=0.999))
    print("%s_ex n %d: worst error / bracket %.3f" % (kind, n, worst))
    assert worst <= 1.0


def test_trainer_end_to_end():
    """The recipe on the smallest trainer setup (4 x 3 x 64 x 64, head '512'): RMSprop with momentum 0.9, clipping, the skip and the
    EMA, three steps."""
    from mnasnet_pytorch_amd.train_step import Trainer
    x = C.det_input((4, 3, 64, 64)).cuda()
    t = torch.tensor([1, 3, 5, 7]).cuda()
    m = build("512", 10, proj_gamma=0.1).train()
    _no_dropout(m)
    tr = Trainer(m, lr=1e-3, optimizer="rmsprop", momentum=0.9, clip_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    assert torch.equal(tr.flat_ema, tr.flat_p) and tr.flat_ema.data_ptr() != tr.flat_p.data_ptr()
    losses = [float(tr.step(x, t)) for _ in range(3)]
    st = tr.grad_stats()
    print("trainer: losses", losses, st)
    assert np.isfinite(losses).all() and st.steps == 3 and st.skipped_steps == 0 and np.isfinite(st.last_norm) and st.last_norm > 0
    assert float(tr.last_grad_norm.cpu()[0]) == st.last_norm
    assert not torch.equal(tr.flat_ema, tr.flat_p)

    def logits():
        m.eval()
        with torch.no_grad():
            y = m(x).detach().clone()
        m.train()
        return y

    p_before, e_before = tr.flat_p.clone(), tr.flat_ema.clone()
    outside = logits()
    with tr.ema_weights():
        inside = logits()
        assert torch.equal(tr.flat_p, e_before) and torch.equal(tr.flat_ema, p_before)
    assert not torch.equal(inside, outside)
    assert torch.equal(logits(), outside) and torch.equal(tr.flat_p, p_before) and torch.equal(tr.flat_ema, e_before)
    with pytest.raises(KeyError):
        with tr.ema_weights():
            raise KeyError("body")
    assert torch.equal(logits(), outside) and torch.equal(tr.flat_p, p_before) and torch.equal(tr.flat_ema, e_before)
    # validate_ema() == a hand-rolled swap around validate()
    batches = [(x, t)]
    a = tr.validate_ema(batches)
    with tr.ema_weights():
        b = tr.validate(batches)
    plain = tr.validate(batches)
    assert (a.loss.avg, a.acc[1].avg, a.samples) == (b.loss.avg, b.acc[1].avg, b.samples) and a.loss.avg != plain.loss.avg
    assert m.training and torch.equal(tr.flat_p, p_before)
    # ema_state_dict() loads into a fresh model and reproduces the EMA logits
    sd = tr.ema_state_dict()
    assert torch.equal(tr.flat_p, p_before) and set(sd) == set(m.state_dict())
    m2 = build("512", 10, proj_gamma=0.1)
    m2.load_state_dict(sd)
    m2.eval()
    with torch.no_grad():
        assert torch.equal(m2(x), inside)
    # checkpoint round trip: the shadow comes back bit for bit
    ck = tr.state_dict()
    assert torch.equal(ck["optimizer"]["state"]["ema"], e_before)
    m3 = build("512", 10, proj_gamma=0.1).train()
    _no_dropout(m3)
    tr3 = Trainer(m3, lr=1e-3, optimizer="rmsprop", momentum=0.9, clip_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    tr3.load_state_dict(ck)
    assert torch.equal(tr3.flat_ema, e_before) and tr3.step_count == 3
    # the EMA off: entering raises, the state dict has the old keys
    m4 = build("512", 10, proj_gamma=0.1).train()
    tr4 = Trainer(m4, lr=1e-3)
    with pytest.raises(RuntimeError, match="EMA"):
        with tr4.ema_weights():
            pass
    assert set(tr4.state_dict()["optimizer"]["state"]) == {"step", "exp_avg", "exp_avg_sq"}
