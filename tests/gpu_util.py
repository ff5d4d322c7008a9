"""Helpers for the -m gpu parity tests: thin torch-tensor wrappers over the C ABI (include/mnas.h)."""
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


def guarded(shape, dtype, device="cuda"):
    esz = torch.empty((), dtype=dtype).element_size()
    pad = CANARY_BYTES // esz
    n = 1
    for s in shape:
        n *= int(s)
    raw = torch.full((pad + n + pad,), _FILL[esz], dtype=_RAW[esz], device=device)
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


# ---- fp64 references built from slicing, matmul / einsum and elementwise ops only (no convolution call: nothing goes to a
# vendor convolution library on the device).  NHWC layouts as the kernels use them; `device` is where the fp64 math runs. -------
def _f64(t, device):
    return t.to(device=device, dtype=torch.float64)


def ref_dy(g, y, coef, device="cpu"):
    """dy = c1*g*[s*y+t > 0] + c2*y + c3 over the last (channel) dimension; coef: bnbuf rows 0..4 ([>=5][C])"""
    g, y, cf = _f64(g, device), _f64(y, device), _f64(coef, device)
    s, t, c1, c2, c3 = cf[0], cf[1], cf[2], cf[3], cf[4]
    return c1 * g * ((s * y + t) > 0) + c2 * y + c3


def ref_dw_fwd(x, w, device="cpu"):
    """depthwise k x k, stride 1, pad k//2: x (N,H,W,C), w (C,k,k) -> (N,H,W,C)"""
    x, w = _f64(x, device), _f64(w, device)
    N, H, W, C_ = x.shape
    k = w.shape[-1]
    p = k // 2
    xp = torch.zeros((N, H + 2 * p, W + 2 * p, C_), dtype=torch.float64, device=device)
    xp[:, p:p + H, p:p + W] = x
    y = torch.zeros_like(x)
    for kh in range(k):
        for kw in range(k):
            y += xp[:, kh:kh + H, kw:kw + W] * w[:, kh, kw]
    return y


def ref_dw_dgrad(dy, w, device="cpu"):
    """input gradient of ref_dw_fwd: dy (N,H,W,C) -> (N,H,W,C)"""
    dy, w = _f64(dy, device), _f64(w, device)
    N, H, W, C_ = dy.shape
    k = w.shape[-1]
    p = k // 2
    gp = torch.zeros((N, H + 2 * p, W + 2 * p, C_), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            gp[:, kh:kh + H, kw:kw + W] += dy * w[:, kh, kw]
    return gp[:, p:p + H, p:p + W].contiguous()


def ref_dw_wgrad(x, dy, k, device="cpu"):
    """weight gradient of ref_dw_fwd: x, dy (N,H,W,C) -> (C,k,k)"""
    x, dy = _f64(x, device), _f64(dy, device)
    N, H, W, C_ = x.shape
    p = k // 2
    xp = torch.zeros((N, H + 2 * p, W + 2 * p, C_), dtype=torch.float64, device=device)
    xp[:, p:p + H, p:p + W] = x
    dw = torch.zeros((C_, k, k), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            dw[:, kh, kw] = torch.einsum("nhwc,nhwc->c", xp[:, kh:kh + H, kw:kw + W], dy)
    return dw


def ref_dense_s2_dgrad(dy, w, H, W, device="cpu"):
    """input gradient of a dense 3x3 stride-2 pad-1 conv: dy (N,Ho,Wo,Co), w (Co,Ci,3,3) -> (N,H,W,Ci).  Forward pixel h reads
    input row 2*ho + kh - 1, so tap (kh, kw) scatters dy[ho, wo] @ w[:, :, kh, kw] to padded row 2*ho + kh."""
    dy, w = _f64(dy, device), _f64(w, device)
    N, Ho, Wo, Co = dy.shape
    Ci = w.shape[1]
    Hp, Wp = max(H + 2, 2 * Ho + 1), max(W + 2, 2 * Wo + 1)
    gp = torch.zeros((N, Hp, Wp, Ci), dtype=torch.float64, device=device)
    for kh in range(3):
        for kw in range(3):
            gp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += torch.matmul(dy, w[:, :, kh, kw])
    return gp[:, 1:1 + H, 1:1 + W].contiguous()


def ref_dense_fwd(a, w, bias=None, stride=1, pad=None, device="cpu"):
    """dense k x k conv: a (N,H,W,Ci) (the operand as the kernel sees it), w (Co,Ci,k,k), bias [Co] -> (N,Ho,Wo,Co).
    One matmul per tap over a strided slice of the zero-padded input."""
    a, w = _f64(a, device), _f64(w, device)
    N, H, W, Ci = a.shape
    Co, _, k, _ = w.shape
    p = k // 2 if pad is None else pad
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    if p:
        ap = torch.zeros((N, H + 2 * p, W + 2 * p, Ci), dtype=torch.float64, device=device)
        ap[:, p:p + H, p:p + W] = a
    else:
        ap = a
    y = torch.zeros((N, Ho, Wo, Co), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            y += torch.matmul(ap[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride], w[:, :, kh, kw].t())
    if bias is not None:
        y += _f64(bias, device)
    return y


def ref_dense_dgrad(dy, w, H, W, stride=1, pad=None, device="cpu"):
    """input gradient of ref_dense_fwd: dy (N,Ho,Wo,Co), w (Co,Ci,k,k) -> (N,H,W,Ci) (any stride; ref_dense_s2_dgrad is the
    3x3 stride-2 case of it)"""
    dy, w = _f64(dy, device), _f64(w, device)
    N, Ho, Wo, Co = dy.shape
    Ci, k = w.shape[1], w.shape[2]
    p = k // 2 if pad is None else pad
    Hp, Wp = max(H + 2 * p, (Ho - 1) * stride + k), max(W + 2 * p, (Wo - 1) * stride + k)
    gp = torch.zeros((N, Hp, Wp, Ci), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            gp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] += torch.matmul(dy, w[:, :, kh, kw])
    return gp[:, p:p + H, p:p + W].contiguous()


def ref_dense_wgrad(a, dy, k, stride=1, pad=None, device="cpu"):
    """weight gradient of ref_dense_fwd: a (N,H,W,Ci), dy (N,Ho,Wo,Co) -> (Co,Ci,k,k)"""
    a, dy = _f64(a, device), _f64(dy, device)
    N, H, W, Ci = a.shape
    _, Ho, Wo, Co = dy.shape
    p = k // 2 if pad is None else pad
    ap = torch.zeros((N, H + 2 * p, W + 2 * p, Ci), dtype=torch.float64, device=device)
    ap[:, p:p + H, p:p + W] = a
    dw = torch.zeros((Co, Ci, k, k), dtype=torch.float64, device=device)
    d2 = dy.reshape(-1, Co)
    for kh in range(k):
        for kw in range(k):
            sl = ap[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
            dw[:, :, kh, kw] = d2.t() @ sl.reshape(-1, Ci)
    return dw


def ref_dw_fwd_s(x, w, bias=None, stride=1, device="cpu"):
    """depthwise k x k, pad k//2, stride 1 or 2: x (N,H,W,C), w (C,k,k) -> (N,Ho,Wo,C)"""
    y = ref_dw_fwd(x, w, device)[:, ::stride, ::stride].contiguous()
    if bias is not None:
        y += _f64(bias, device)
    return y


def ref_stem(t, w, bias=None, device="cpu"):
    """the stem conv (3x3, stride 2, pad 1) over the image the kernel stages: t (N,3,H,W) NCHW, w (Co,3,3,3) -> (N,Ho,Wo,Co)"""
    return ref_dense_fwd(t.permute(0, 2, 3, 1), w, bias, stride=2, pad=1, device=device)


def ref_stem_wgrad(t, dy, device="cpu"):
    """t (N,3,H,W), dy (N,Ho,Wo,Co) -> (Co,3,3,3)"""
    return ref_dense_wgrad(t.permute(0, 2, 3, 1), dy, 3, stride=2, pad=1, device=device)


def check_gemm_bound(hip, ref, S, K, what):
    """Per-element bound for a GEMM launch whose operands need no transform on load (plain activation, materialised dy).
    hip: the bf16 output; ref: the fp64 result over the same bf16 operands; S = |bias| + sum |a|*|w| (the same reference on
    absolute values); K: reduction length.  Derivation: a product of two bf16 numbers is exact in fp32; each of the K
    accumulations (and the bias add) loses at most 2^-23 relative to the running magnitude <= S, rounding toward zero
    included, so the fp32 result is within (K+1)*2^-23*S of ref; the bf16 store (round to nearest even, 8 significand bits)
    adds at most half an ulp, which is at most 2^-8*|value| (reached just above a power of two; 2^-9 just below one).
    Asserted for EVERY element: |hip - ref| <= 2^-8*|ref| + (K+1)*2^-22*S -- the store term is the exact worst case, the
    accumulation term carries a factor of two (it also absorbs a value that the fp32 error moves across a rounding
    boundary or a power of two).  Correct kernels were measured at up to 0.99 of this bound.  Not covered: an operand
    formed on load (act-on-load, dy-on-load) -- one bf16 ulp of an operand computed in fp32 on the device and in fp64 on
    the host is outside this derivation; those launches keep the max-normalised tolerance."""
    hip, ref, S = hip.double(), ref.double(), S.double()
    assert hip.shape == ref.shape == S.shape, (what, hip.shape, ref.shape, S.shape)
    err = (hip - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + (K + 1) * 2.0 ** -22 * S
    bad = ~(err <= bound)                     # (a NaN fails)
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside the per-element bound; first at %s: got %r, fp64 %r, |err| %.3e > bound %.3e"
                             % (what, int(bad.sum()), bad.numel(), idx, float(hip[idx]), float(ref[idx]), float(err[idx]), float(bound[idx])))
    return float((err / bound.clamp_min(1e-300)).max())
