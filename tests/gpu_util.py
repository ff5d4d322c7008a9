"""Launch side of the -m gpu parity tests: thin torch-tensor wrappers over the C ABI (include/mnas.h), guarded output buffers and
bit comparison -- a minimal worked example of the ABI.  The fp64 references are in refs64.py, the per-element error bounds in
intervals.py and bounds_*.py."""
import ctypes as C

import torch

from mnasnet_pytorch_amd import _lib as L


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nhwc(x):
    """NCHW fp32 (cpu) -> NHWC bf16 cuda"""
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()


def from_nhwc(t):
    """NHWC bf16 cuda -> NCHW fp32 cpu"""
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def act_in(data, scale=None, shift=None):
    return L.MnasActIn(L.ptr(data), L.ptr(scale), L.ptr(shift))


def grad_in(g, y, coef):
    return L.MnasGradIn(L.ptr(g), L.ptr(y), L.ptr(coef))


def pack(w, kind):
    """w: reference-layout fp32 weight (cpu or cuda) -> packed device buffer"""
    lib = L.load()
    w = w.detach().float().cuda().contiguous()
    Co, Cig, kh, kw = w.shape
    Ci = Cig
    nbytes = lib.mnas_packed_bytes(kind, Co, Ci, kh, kw)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    L.check(lib.mnas_pack_weights(w.data_ptr(), kind, Co, Ci, kh, kw, dst.data_ptr(), L.cur_stream()), "pack")
    return dst


def gemm_args(mode, N, Hi, Wi, Ci, Ho, Wo, Co, k, stride, pad, nparts=64):
    """MnasConvGemm with the integers set and every pointer NULL"""
    a = L.MnasConvGemm()
    a.mode, a.N, a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.Co = mode, N, Hi, Wi, Ci, Ho, Wo, Co
    a.kh = a.kw = k
    a.stride, a.pad, a.nparts = stride, pad, nparts
    return a


ROUTES = {L.ROUTE_PWX: "k_pwx", L.ROUTE_PWS: "k_pws", L.ROUTE_PWF: "k_pwf", L.ROUTE_PWD: "k_pwd", L.ROUTE_C3R: "k_c3r",
          L.ROUTE_DIMG: "k_dimg", L.ROUTE_C3X: "k_c3x", L.ROUTE_IGEMM: "k_igemm"}


def conv_gemm_route(a):
    """(route name, (NT, PT, k-chunk, parity-class form)) mnas_conv_gemm picks for `a`; the instance is zeros unless k_igemm.
    Only the integers and which pointers are non-NULL matter: host-side, nothing is read or launched."""
    inst = (C.c_int * 4)()
    r = L.load().mnas_conv_gemm_route(C.byref(a), inst)
    assert r >= 0, "mnas_conv_gemm_route: %d" % r
    return ROUTES[r], tuple(inst)


def route_of(mode, N, Hi, Wi, Ci, Ho, Wo, Co, k, stride, pad, virt=True, coef=True, resid=False, gate=False, bias=True):
    """route for a launch described by its integers and pointer-presence flags (any non-NULL value stands for a pointer)"""
    a = gemm_args(mode, N, Hi, Wi, Ci, Ho, Wo, Co, k, stride, pad)
    one = 64
    if mode == 0:
        a.act = L.MnasActIn(one, one if virt else 0, one if virt else 0)
        a.bias = one if bias else 0
    else:
        a.grad = L.MnasGradIn(one, one if coef else 0, one if coef else 0)
    a.resid = one if resid else 0
    a.gate = one if gate else 0
    a.w = a.out = one
    return conv_gemm_route(a)


def conv_gemm(mode, N, Hi, Wi, Ci, Ho, Wo, Co, k, stride, pad, w, bias=None, act=None, grad=None, resid=None,
              nparts=64, stats=False, red_y=None, red_bn=None, gate=None, expect=0, guard=False, route=None):
    """guard: out and stats live in guarded() buffers and are check()ed after the launch; route: (name, instance) sink list --
    the dispatcher's answer for exactly this struct is appended to it"""
    lib = L.load()
    if guard:
        out, ochk = guarded((N, Ho, Wo, Co), torch.bfloat16)
        st, schk = guarded((2, Co, nparts), torch.float32) if stats else (None, None)
    else:
        out = torch.empty((N, Ho, Wo, Co), dtype=torch.bfloat16, device="cuda")
        st = torch.full((2, Co, nparts), float("nan"), device="cuda") if stats else None
    a = gemm_args(mode, N, Hi, Wi, Ci, Ho, Wo, Co, k, stride, pad, nparts)
    if act is not None:
        a.act = act
    if grad is not None:
        a.grad = grad
    a.w, a.bias, a.resid, a.out, a.stats = L.ptr(w), L.ptr(bias), L.ptr(resid), L.ptr(out), L.ptr(st)
    a.red_y, a.red_bn = L.ptr(red_y), L.ptr(red_bn)
    a.gate = L.ptr(gate)
    if route is not None:
        route.append(conv_gemm_route(a))
    rc = lib.mnas_conv_gemm(C.byref(a), L.cur_stream())
    if expect:
        assert rc == expect, rc
        return None, None
    L.check(rc, "conv_gemm")
    if guard:
        what = "conv_gemm mode %d %s k%d s%d -> %d nparts %d" % (mode, (N, Hi, Wi, Ci), k, stride, Co, nparts)
        ochk(what + " out")
        if stats:
            schk(what + " stats")
    return out, st


def rand_bn_coefs(C, seed, O):
    """Plausible (s,t,c1,c2,c3,mean,invstd,_) rows for dy-on-load tests; returns [8][C] fp32 cpu"""
    u = O.det_uniform((8, C), seed)
    b = torch.zeros(8, C)
    b[0] = 1.0 + 0.3 * u[0]          # s
    b[1] = 0.2 * u[1]                # t
    b[2] = b[0]                      # c1 = s
    b[3] = 0.05 * u[3]               # c2
    b[4] = 0.02 * u[4]               # c3
    b[5] = 0.1 * u[5]                # mean
    b[6] = 1.0 + 0.2 * u[6].abs()    # invstd
    return b


def dy_ref(g, y, b, rounded=True):
    """g,y: NCHW fp32 (already bf16-rounded); b: [8][C].  Returns dy as the kernels use it: bf16-rounded where it is
    staged into LDS for the MFMA kernels, fp32 for the depthwise kernels (which form it on the fly from raw g, y)."""
    s, t, c1, c2, c3 = (b[i].view(1, -1, 1, 1) for i in range(5))
    dz = g * ((s * y + t) > 0)
    d = c1 * dz + c2 * y + c3
    return bf16r(d) if rounded else d


# ---- guarded output buffers ----------------------------------------------------------------------------------------------
# A kernel's output view sits inside a larger buffer filled with a NaN bit pattern that no kernel produces (the canonical NaN is
# 0x7fc0 / 0x7fc00000).  check(): the canaries before and after the view are bit-unchanged (no write outside the tensor) and no
# element of the view still holds the pattern (every element was written: what "fully overwritten" in include/mnas.h promises).
_FILL = {2: 0x7FA5, 4: 0x7FA5A5A5}
_RAW = {2: torch.int16, 4: torch.int32}
CANARY_BYTES = 4096


def guarded(shape, dtype, device="cuda", offset=0):
    """offset: the view starts that many ELEMENTS behind the (16-byte aligned) end of the leading canary -- a tensor at a 4-byte,
    not 16-byte, aligned address; the skipped elements count as canary"""
    esz = torch.empty((), dtype=dtype).element_size()
    pad = CANARY_BYTES // esz + offset
    n = 1
    for s in shape:
        n *= int(s)
    raw = torch.full((pad + n + CANARY_BYTES // esz,), _FILL[esz], dtype=_RAW[esz], device=device)
    view = raw[pad:pad + n].view(dtype).view(*shape)

    def check(what="output", written=True):
        fill = _FILL[esz]
        assert bool((raw[:pad] == fill).all()), "%s: write before the tensor (leading canary changed)" % what
        assert bool((raw[pad + n:] == fill).all()), "%s: write past the end of the tensor (trailing canary changed)" % what
        if written:
            left = raw[pad:pad + n] == fill
            if bool(left.any()):
                idx = int(left.nonzero()[0])
                raise AssertionError("%s: %d of %d elements never written (first: flat index %d of shape %s)"
                                     % (what, int(left.sum()), n, idx, tuple(shape)))
    return view, check


def bits_equal(a, b, what="tensor", signed_zero=True):
    """Bit-for-bit comparison of two tensors of one dtype; signed_zero=False counts +0 and -0 as equal.  The message names the
    first differing element (index in the tensor's own shape)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    esz = a.element_size()
    ra, rb = a.contiguous().view(_RAW[esz]), b.contiguous().view(_RAW[esz])
    if not signed_zero:
        sign = -(1 << (8 * esz - 1))
        ra = torch.where(ra == sign, torch.zeros_like(ra), ra)
        rb = torch.where(rb == sign, torch.zeros_like(rb), rb)
    diff = ra != rb
    if bool(diff.any()):
        flat = int(diff.reshape(-1).nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), a.shape))
        raise AssertionError("%s: %d of %d elements differ in their bits; first at %s: %r vs %r"
                             % (what, int(diff.sum()), diff.numel(), idx, float(a[idx]), float(b[idx])))
