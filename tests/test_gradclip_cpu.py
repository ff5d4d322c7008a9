"""CPU (no GPU needed): the numpy helper of the clipping arithmetic (tests/gradclip_ref.py) against torch.nn.utils.clip_grad_norm_,
the four new C-ABI symbols with their ctypes mirrors, and the optimizers' argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gradclip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e3])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_helper_is_torchs_clip_grad_norm(max_norm, grad_scale):
    """Same quantity as torch's, not the same bits: torch sums the squares in fp32 in another order, the helper in float64 with one
    rounding.  Moderate magnitudes (|g| ~ 1, 3 tensors, 12k elements): norm, coefficient and clipped gradient to 2^-20 relative."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(10007,), (33, 65), (7,)]
    grads = [torch.randn(s, generator=gen) * (0.3 + 0.4 * i) for i, s in enumerate(shapes)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for p, g in zip(params, grads):
        p.grad = (g * grad_scale).clone()                  # what the optimizer consumes: the fp32 product
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    flat = np.concatenate([g.numpy().ravel() for g in grads])
    n, c, gc = R.clipped(flat, max_norm, grad_scale)
    assert abs(float(n) - float(total)) <= 2.0 ** -20 * float(total)
    c_torch = min(1.0, max_norm / (float(total) + 1e-6))
    assert abs(float(c) - c_torch) <= 2.0 ** -20 * c_torch
    got = np.concatenate([p.grad.numpy().ravel() for p in params])
    assert np.abs(gc - got).max() <= 2.0 ** -20 * np.abs(got).max()
    assert (float(c) < 1.0) == (float(total) > max_norm)
    # several runs = the norm of the concatenation
    assert R.norm([flat[:5000], flat[5000:]], grad_scale) == n


def test_helper_edge_values():
    assert R.norm(np.zeros(100, np.float32)) == 0 and R.coef(np.float32(0), 1.0) == 1           # 1 / 1e-6 clamps to 1
    big = R.norm(np.full(1000, 1e25, np.float32))
    assert np.isfinite(big) and abs(float(big) - 1e25 * np.sqrt(1000.0)) <= 2.0 ** -22 * float(big)
    assert np.isnan(R.coef(np.float32(np.nan), 1.0)) and R.coef(np.float32(np.inf), 1.0) == 0   # torch.clamp keeps the NaN
    for off in (None, 0.0, -1.0, float("inf")):
        assert R.coef(np.float32(7.0), off) == 1
    v, b = R.ema_bound(0.9, np.float32([1.0]), np.float32([2.0]))
    assert abs(v[0] - 1.1) < 1e-7 and 0 < b[0] < 3e-7


def test_library_exports_the_new_symbols():
    from mnasnet_pytorch_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mnas.h")).read()
    nargs = {"mnas_grad_sqnorm": 7, "mnas_adam_step_ex": 14, "mnas_rmsprop_step_ex": 13, "mnas_sgd_step_ex": 13}
    for name, k in nargs.items():
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
        assert len(_lib.SYMBOLS[name][1]) == k, name
        plain = name[:-3]
        if name.endswith("_ex"):                            # the plain entry point's arguments plus the MnasOptExtra pointer
            assert _lib.SYMBOLS[name][1][:-2] == _lib.SYMBOLS[plain][1][:-1]
            assert _lib.SYMBOLS[name][1][-2] is ctypes.POINTER(_lib.MnasOptExtra)
    assert lib.mnas_version() == _lib.ABI_VERSION == 8       # additive: the version does not move
    assert int(re.search(r"#define MNAS_GRADNORM_MAX_PARTS\s+(\d+)", hdr).group(1)) == _lib.GRADNORM_MAX_PARTS == 1024


def _c_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"([\w ]+?\*?)\s+(\w+);", body)


def test_struct_mirrors_match_header():
    from mnasnet_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mnas.h")).read()
    ctype = {"float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    for name, cls, size in (("MnasGradStats", _lib.MnasGradStats, 32), ("MnasOptExtra", _lib.MnasOptExtra, 56)):
        fields = [(" ".join(t.split()), n) for t, n in _c_fields(hdr, name)]
        assert [n for _, n in fields] == [n for n, _ in cls._fields_], name
        for (t, n), (_, ct) in zip(fields, cls._fields_):
            assert ct is (ctypes.c_void_p if t.endswith("*") else ctype[t]), (name, n)
        assert ctypes.sizeof(cls) == size, name
    S = _lib.MnasGradStats
    assert (S.last_norm.offset, S.last_coef.offset, S.steps.offset, S.clipped_steps.offset, S.skipped_steps.offset) == (0, 4, 8, 16, 24)


def test_entry_points_check_their_arguments_on_the_host():
    """Every bad argument is refused on the host, before a launch (a CPU test: the calls that succeed are empty runs)."""
    from mnasnet_pytorch_amd import _lib
    lib, E = _lib.load(), _lib.EINVAL
    got = ctypes.c_int(-1)
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    assert lib.mnas_grad_sqnorm(None, 8, 1.0, a, 0, ctypes.byref(got), None) == E
    assert lib.mnas_grad_sqnorm(a, 8, 1.0, None, 0, ctypes.byref(got), None) == E
    assert lib.mnas_grad_sqnorm(a, -1, 1.0, a, 0, ctypes.byref(got), None) == E
    assert lib.mnas_grad_sqnorm(a, 8, 1.0, a, -1, ctypes.byref(got), None) == E
    assert lib.mnas_grad_sqnorm(a, 8, 1.0, a, 1024, ctypes.byref(got), None) == E            # 1024 + 1 slot
    assert lib.mnas_grad_sqnorm(a, 1 << 20, 1.0, a, 1024 - 255, ctypes.byref(got), None) == E  # 256 slots from 769
    assert got.value == -1
    assert lib.mnas_grad_sqnorm(a, 0, 1.0, a, 1024, ctypes.byref(got), None) == 0 and got.value == 0   # empty run: no launch

    def extra(**kw):
        base = dict(partial=a, nparts=1, max_norm=1.0, skip_nonfinite=0, ema=None, ema_decay=0.0, stats=a, update_stats=1)
        base.update(kw)
        return ctypes.byref(_lib.MnasOptExtra(**base))

    def adam(ex, n=4, p=a):
        return lib.mnas_adam_step_ex(p, a, a, a, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, ex, None)

    def rms(ex, n=4):
        return lib.mnas_rmsprop_step_ex(a, a, a, None, n, 1e-3, 0.99, 1e-8, 0.0, 0.0, 1.0, ex, None)

    def sgd(ex, n=4):
        return lib.mnas_sgd_step_ex(a, a, None, n, 1e-3, 0.0, 0.0, 0.0, 0, 1, 1.0, ex, None)

    for fn in (adam, rms, sgd):
        assert fn(None) == E
        assert fn(extra(), n=-1) == E
        assert fn(extra(nparts=1025)) == E and fn(extra(nparts=-1)) == E
        assert fn(extra(partial=None)) == E
        assert fn(extra(ema=a, ema_decay=1.0)) == E and fn(extra(ema=a, ema_decay=-0.1)) == E
        assert fn(extra(ema=a, ema_decay=float("nan"))) == E
        assert fn(extra(stats=None)) == E
        assert fn(extra(nparts=0, partial=None)) == E                       # clipping without a norm
        assert fn(extra(nparts=0, partial=None, max_norm=0.0, skip_nonfinite=1)) == E
        assert fn(extra(max_norm=float("nan"))) == E
        assert fn(extra(), n=0) == 0                                        # valid and empty: no launch
        assert fn(extra(nparts=0, partial=None, max_norm=float("inf"), ema=a, ema_decay=0.5), n=0) == 0     # EMA only
    assert adam(extra(), p=None) == E


def _cpu_opt(cls, n=64, **kw):
    flat_p, flat_g = torch.zeros(n), torch.zeros(n)
    par = torch.nn.Parameter(flat_p.view(n))
    par.data = flat_p.view(n)
    return cls([par], flat_p, flat_g, **kw)


@pytest.mark.parametrize("kind", ["adam", "rmsprop", "sgd"])
def test_constructor_validation_and_state_dict_keys(kind):
    from mnasnet_pytorch_amd.train_step import FlatAdam, FlatRMSprop, FlatSGD
    cls = {"adam": FlatAdam, "rmsprop": FlatRMSprop, "sgd": FlatSGD}[kind]
    with pytest.raises(ValueError, match="ema_decay"):
        _cpu_opt(cls, ema_decay=1.0)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        _cpu_opt(cls, clip_grad_norm=-1)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        _cpu_opt(cls, clip_grad_norm=0.0)
    opt = _cpu_opt(cls)
    assert (opt.clip_grad_norm, opt.skip_nonfinite, opt.ema_decay, opt.flat_ema) == (None, False, None, None)
    assert set(opt.state_dict()["state"]) == {"step", "exp_avg", "exp_avg_sq"}        # the EMA off: the keys as they were
    on = _cpu_opt(cls, clip_grad_norm=2.0, skip_nonfinite=True, ema_decay=0.9999)
    assert on.flat_ema is not None and on.flat_ema.data_ptr() != on.flat_p.data_ptr() and torch.equal(on.flat_ema, on.flat_p)
    sd = on.state_dict()
    assert set(sd["state"]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
    # plain attributes, checked again when a step reads them
    on.ema_decay = 1.5
    with pytest.raises(ValueError, match="ema_decay"):
        on.step()
    # load: the shadow comes from the checkpoint; without the key and with the EMA on it restarts from the parameters
    on.ema_decay = 0.5
    sd["state"]["ema"] = torch.full_like(on.flat_p, 3.0)
    on.load_state_dict(sd)
    assert bool((on.flat_ema == 3.0).all())
    on.flat_p.fill_(7.0)
    on.load_state_dict(opt.state_dict())
    assert bool((on.flat_ema == 7.0).all())
    off = _cpu_opt(cls)
    off.load_state_dict(sd)                                   # a checkpoint with a shadow into an optimizer with the EMA off: kept
    assert bool((off.flat_ema == 3.0).all()) and "ema" not in off.state_dict()["state"]


def test_trainer_surface():
    import inspect
    from mnasnet_pytorch_amd.train_step import GradStats, Trainer
    assert GradStats._fields == ("last_norm", "last_coef", "steps", "clipped_steps", "skipped_steps")
    for name in ("grad_stats", "ema_weights", "ema_state_dict", "last_grad_norm", "validate_ema"):
        assert hasattr(Trainer, name), name
    # validate under the EMA weights is a method of its own with validate's parameters (validate's signature is pinned elsewhere)
    assert list(inspect.signature(Trainer.validate_ema).parameters) == list(inspect.signature(Trainer.validate).parameters)
