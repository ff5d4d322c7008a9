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
    boundary or a power of two).  Correct kernels were measured at up to 0.99 of this bound.  An operand formed on load
    (act-on-load, dy-on-load) is outside this derivation: check_onload_bound below is this bound plus the operand's
    interval.  The squeeze-excite kernels and the gated act-on-load (act8g), the stem's weight and input gradients,
    mnas_add_act / the pooling glue and the finalizes have their own helpers at the end of this file."""
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


# ---- per-element bounds for launches whose operand is formed on load, for the depthwise sweeps and for fp32 sums ------------------
# u = 2^-24 is the unit roundoff of fp32 (round to nearest).  The host never re-enacts the device's fp32 evaluation of an operand: it
# brackets it in fp64 by an interval [lo, hi] that every correctly rounded evaluation (fused or not) falls into, and carries the
# interval's half width through the reference as `slack`.  Nothing here is fitted to a kernel's output.
U32 = 2.0 ** -24
HINGE = 1e-3            # inputs are moved off the ReLU hinge |s*v+t| < HINGE: host and device then agree on every mask bit
MAX_ACT_SPLIT = 1e-3    # largest share of bf16 activation operand elements whose interval straddles a bf16 rounding boundary
MAX_DY_SPLIT = 2e-2     # the same for a dy operand (it cancels: three terms of either sign)
MAX_HINGE_MOVED = 1e-2  # largest share of elements off_hinge may move


def _pre(v, s, t):
    return s.double().to(v.device) * v.double() + t.double().to(v.device)


def _on_hinge(v, s, t):
    """|s*v+t| < HINGE, except where v == 0 and t == 0: there s*v+t is exactly zero in fp32 and in fp64 alike"""
    exact0 = (v.double() == 0) & (t.double().to(v.device) == 0).expand_as(v)
    return (_pre(v, s, t).abs() < HINGE) & ~exact0


def off_hinge(v, s, t):
    """v (..., C) fp32 holding bf16 values; s, t [C]: move the elements with |s*v+t| < HINGE to where s*v+t ~ +0.05 (bf16).
    An element with v == 0 under t == 0 stays: its s*v+t is the exact zero on host and device.  At most MAX_HINGE_MOVED of the
    elements may need moving (a test whose inputs sit on the hinge wholesale is testing something else)."""
    sd, td = s.double().to(v.device), t.double().to(v.device)
    bad = _on_hinge(v, s, t)
    share = float(bad.double().mean())
    assert share <= MAX_HINGE_MOVED, "off_hinge would move %.3g of the elements (limit %.3g)" % (share, MAX_HINGE_MOVED)
    alt = bf16r(((0.05 - td) / sd).float()).expand_as(v)
    out = torch.where(bad, alt, v)
    assert not bool(_on_hinge(out, s, t).any())
    off_hinge.worst = max(off_hinge.worst, share)
    return out


off_hinge.worst = 0.0


def zero_on_hinge(g, y, s, t):
    """Where y cannot be moved (it is another kernel's output, e.g. the forward's stored y that RECOMP recomputes): g = 0 at the
    elements with y on the hinge, so that g*[s*y+t > 0] = 0 whichever way the mask bit falls.  Same share limit as off_hinge."""
    bad = _on_hinge(y, s, t)
    share = float(bad.double().mean())
    assert share <= MAX_HINGE_MOVED, "zero_on_hinge would clear %.3g of the elements (limit %.3g)" % (share, MAX_HINGE_MOVED)
    off_hinge.worst = max(off_hinge.worst, share)
    return torch.where(bad, torch.zeros_like(g), g)


def relu_mask(v, s, t):
    """[s*v+t > 0] in fp64; v must be off the hinge (off_hinge), so the device's fp32 fma (within u*|s*v+t|) gives the same bits"""
    assert not bool(_on_hinge(v, s, t).any()), "mask input on the ReLU hinge: move it with off_hinge first"
    return _pre(v, s, t) > 0


def _bf16_64(t):
    """fp64 -> fp32 -> bf16 (both round to nearest even) -> fp64: monotone, so it maps an interval's ends to the ends of the
    interval of rounded values"""
    return t.float().to(torch.bfloat16).double()


class Interval:
    """an operand tensor known to lie in [lo, hi] element by element (fp64)"""
    worst_act = 0.0      # largest measured shares of split bf16 elements
    worst_dy = 0.0

    def __init__(self, lo, hi, D=None, val=None):
        """D: the magnitude the operand's rounding is relative to; val: the exact (fp64) value of the operand"""
        assert bool((lo <= hi).all())
        self.lo, self.hi, self.D, self.val = lo, hi, D, val

    @staticmethod
    def exact(x, device=None):
        x = x.double() if device is None else _f64(x, device)
        return Interval(x, x, x.abs(), x)

    @property
    def mid(self):
        return (self.lo + self.hi) / 2

    @property
    def half(self):
        return (self.hi - self.lo) / 2

    @property
    def amax(self):
        return torch.maximum(self.lo.abs(), self.hi.abs())

    def split_share(self):
        return float((self.lo != self.hi).double().mean())


def act_interval(z, s, t, bf16, device="cpu"):
    """Interval of the act-on-load operand relu(s*z+t) over the last (channel) dimension; z holds bf16 values, s, t fp32.
    Exact value pre = s*z+t (fp64).  The device evaluates one fmaf (act8, dw_act_raw: within u*|pre| <= u*(|s||z|+|t|)); an
    unfused evaluation rounds the product and the sum (within 2u*(|s||z|+|t|) to first order), so eps = 2u*(|s||z|+|t|) covers
    both.  relu is monotone: an fp32 operand (the depthwise sweeps) lies in [relu(pre-eps), relu(pre+eps)].  bf16=True: the MFMA
    kernels round it to bf16 (pack_bf16, round to nearest even), which is monotone too: [bf16(relu(pre-eps)), bf16(relu(pre+eps))].
    Asserted: at most MAX_ACT_SPLIT of the bf16 elements have lo != hi (the interval straddles a rounding boundary).
    .D = |s||z|+|t|, the magnitude the depthwise bound's S is built from."""
    z, s, t = _f64(z, device), _f64(s, device), _f64(t, device)
    pre = s * z + t
    D = s.abs() * z.abs() + t.abs()
    eps = 2 * U32 * D
    lo, hi = torch.relu(pre - eps), torch.relu(pre + eps)
    if bf16:
        lo, hi = _bf16_64(lo), _bf16_64(hi)
    iv = Interval(lo, hi, D, torch.relu(pre))
    if bf16:
        share = iv.split_share()
        assert share <= MAX_ACT_SPLIT, "act operand: %.3g of the bf16 elements straddle a rounding boundary (limit %.3g)" % (share, MAX_ACT_SPLIT)
        Interval.worst_act = max(Interval.worst_act, share)
    return iv


def dy_interval(g, y, coef, bf16, device="cpu", g_masked=False):
    """Interval of the dy-on-load operand dy = c1*g*[s*y+t > 0] + c2*y + c3 (coef rows 0..4) over the last dimension; g, y hold
    bf16 values.  y must be off the ReLU hinge (asserted; an element with g == 0 is exempt: its dz is 0 under either mask bit), so
    the mask bit is the device's.  With D = |c1||g| +
    |c2||y| + |c3|: dy8 / dw_read_dy evaluate fma(c1, dz, fma(c2, y, c3)) -- two nested roundings, within 2u*D -- and an unfused
    evaluation twice as many: eps = 4u*D.  fp32 operand (depthwise): [dy-eps, dy+eps]; bf16=True (pack8 of dy8 in the MFMA
    kernels): both ends rounded to bf16.  Asserted: at most MAX_DY_SPLIT of the bf16 elements have lo != hi.
    g_masked: g already holds g*mask (the g_masked form of mnas_dw_bwd), no mask is applied."""
    g, y, cf = _f64(g, device), _f64(y, device), _f64(coef, device)
    s, t, c1, c2, c3 = cf[0], cf[1], cf[2], cf[3], cf[4]
    if not g_masked:
        assert not bool((_on_hinge(y, s, t) & (g != 0)).any()), "dy-on-load: y on the ReLU hinge under a non-zero g (off_hinge / zero_on_hinge)"
    dz = g if g_masked else g * (s * y + t > 0)
    d = c1 * dz + c2 * y + c3
    D = c1.abs() * g.abs() + c2.abs() * y.abs() + c3.abs()
    eps = 4 * U32 * D
    lo, hi = d - eps, d + eps
    if bf16:
        lo, hi = _bf16_64(lo), _bf16_64(hi)
    iv = Interval(lo, hi, D, d)
    if bf16:
        share = iv.split_share()
        assert share <= MAX_DY_SPLIT, "dy operand: %.3g of the bf16 elements straddle a rounding boundary (limit %.3g)" % (share, MAX_DY_SPLIT)
        Interval.worst_dy = max(Interval.worst_dy, share)
    return iv


WORST = {}          # family -> largest measured error / bound (printed by the tests; DESIGN.md section 6 records them)


def _assert_bound(hip, ref, bound, what, family):
    hip, ref, bound = hip.double(), ref.double(), bound.double()
    assert hip.shape == ref.shape == bound.shape, (what, hip.shape, ref.shape, bound.shape)
    err = (hip - ref).abs()
    bad = ~(err <= bound)                     # (a NaN fails)
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        idx = tuple(int(v) for v in torch.unravel_index(ratio.reshape(-1).argmax(), ratio.shape)) if ratio.dim() else ()
        raise AssertionError("%s: %d of %d elements outside the per-element bound; worst at %s: got %r, fp64 %r, |err| %.3e > bound %.3e (x%.2f)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(hip[idx]), float(ref[idx]), float(err[idx]),
                                float(bound[idx]), float(err[idx] / bound[idx].clamp_min(1e-300))))
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    if family:
        WORST[family] = max(WORST.get(family, 0.0), worst)
    return worst


def onload_elem_err(slack, S, K):
    """what the fp32 value in the accumulator (before the bf16 store) may differ from the fp64 reference by: (K+1)*2^-22*S + slack"""
    return (K + 1) * 2.0 ** -22 * S.double() + slack.double()


def check_onload_bound(hip, ref, slack, S, K, what, family="mfma on-load"):
    """Per-element bound for an MFMA launch (bf16 output) whose operand is formed on load and known as an Interval `a` (bf16 ends).
    ref = conv(a.mid, w) (+bias, +resid); slack = conv(a.half, |w|): how far the exact result over ANY operand inside the
    interval can lie from ref; S = conv(a.amax, |w|) + |bias| + |resid|.  As check_gemm_bound: bf16 x bf16 products are exact,
    K accumulations and the bias / residual add lose (K+1)*2^-23*S, doubled; the bf16 store rounds a value of at most
    |ref|+slack (+ the fp32 error, which the doubled accumulation term absorbs) by at most 2^-8 of it.  EVERY element:
        |hip - ref| <= 2^-8*(|ref| + slack) + (K+1)*2^-22*S + slack.
    With lo == hi everywhere (slack = 0) this is check_gemm_bound."""
    bound = 2.0 ** -8 * (ref.double().abs() + slack.double()) + onload_elem_err(slack, S, K)
    return _assert_bound(hip, ref, bound, what, family)


def dw_elem_err(S, k):
    """fp32 error of a depthwise accumulator before its bf16 store: (2k^2+2)*2^-23*S"""
    return (2 * k * k + 2) * 2.0 ** -23 * S.double()


def check_dw_bound(hip, ref, S, k, what, family="depthwise"):
    """Per-element bound for the depthwise sweeps (fp32 operands formed on read, fp32 weights as given -- NOT rounded to bf16 by
    the test --, k*k taps accumulated in fp32, bf16 output).  ref: the fp64 result over the exact operands (relu(s*z+t) resp. dy in
    fp64).  S: the same sum over magnitudes -- forward |bias| + sum (|s||z|+|t|)*|w| (act_interval(...).D), input gradient
    sum D*|w| (dy_interval(...).D).  Each tap is one fma rounding (or a multiply and an add rounding), 2^-24 of a running
    magnitude <= S each: at most 2k^2*2^-24*S; the operand's own rounding (u resp. 2u of its magnitude, act_interval /
    dy_interval) is at most 2*2^-24*S more; doubled as in check_gemm_bound: (2k^2+2)*2^-23*S.  The bf16 store adds 2^-8*|value|.
        |hip - ref| <= 2^-8*|ref| + (2k^2+2)*2^-23*S      for EVERY element."""
    bound = 2.0 ** -8 * ref.double().abs() + dw_elem_err(S, k)
    return _assert_bound(hip, ref, bound, what, family)


def check_sum_bound(hip, ref, S, M, P, c, what, slack=None, family="fp32 sums"):
    """Bound for an fp32 sum of M terms per output, written as P partial slabs / columns that a finalize (or the host) adds:
    weight-gradient partials after mnas_wgrad_finalize, BatchNorm statistics (sum y, sum y^2), the fused reduce (sum dz,
    sum dz*xhat).  ref: the fp64 sum; S: the same sum over absolute values.  Every add loses at most 2^-24 of a running
    magnitude <= S (M in the kernel, P in the finalize, 1 for an accumulate target or bias); a term that is itself rounded (c = 2:
    fp32 x fp32 products of the depthwise weight gradient, xhat = fma(y, inv, m), y^2) doubles the per-term loss, an exact term
    (c = 1: bf16 x bf16) does not; the whole is doubled as in check_gemm_bound:
        |hip - ref| <= (c*M + P + 1)*2^-22*S + slack.
    slack: what the exact sum over any operands inside their intervals may differ from ref by -- for two interval operands a, b
    sum(|a.mid|*b.half + |b.mid|*a.half + a.half*b.half) (prod_slack); for statistics of an fp32 accumulator, the sum of the
    elements' own fp32 error (onload_elem_err / dw_elem_err)."""
    bound = (c * M + P + 1) * 2.0 ** -22 * S.double()
    if slack is not None:
        bound = bound + slack.double()
    return _assert_bound(hip, ref, bound, what, family)


def stats_bound_terms(ref, e, dims=None):
    """BatchNorm statistics of an fp32 accumulator v with |v - ref| <= e element by element (the kernels sum the accumulator, not
    the stored bf16 value: mnas_stat2 / `s1 += v; s2 = fma(v, v, s2)` sit before pack_bf16 in every forward epilogue).  Returns
    (ref1, S1, slack1, ref2, S2, slack2) per channel for check_sum_bound: sum v against sum ref with slack sum e; sum v^2 against
    sum ref^2 with slack sum (2|ref|e + e^2); S over (|ref|+e) resp. its square."""
    ref, e = ref.double(), e.double()
    dims = tuple(range(ref.dim() - 1)) if dims is None else dims
    a = ref.abs() + e
    return (ref.sum(dims), a.sum(dims), e.sum(dims), (ref * ref).sum(dims), (a * a).sum(dims), (2 * ref.abs() * e + e * e).sum(dims))


def check_stats_bound(st, ref, e, M, what, family="statistics"):
    """st: the [2][C][P] table of a forward launch; ref (..., C): fp64 reference elements; e: their fp32 error bound.  c = 1 for
    sum v, c = 2 for sum v^2 (the square is rounded)."""
    P = st.shape[-1]
    p = st.double().sum(-1)
    r1, S1, k1, r2, S2, k2 = stats_bound_terms(ref, e)
    a = check_sum_bound(p[0].to(r1.device), r1, S1, M, P, 1, what + " stats sum", k1, family)
    b = check_sum_bound(p[1].to(r1.device), r2, S2, M, P, 2, what + " stats sum of squares", k2, family)
    return max(a, b)


def check_red_bound(table, gq, yin, bn, M, what, family="fused reduce"):
    """Fused BatchNorm-backward reduce (sum dz, sum dz*xhat) per channel; table [2][C][P].  The kernels sum the gradient AS STORED
    (mnas_red2 takes the packed bf16 pair; dw: f2bf(pk)): gq is the launch's own bf16 output, yin the raw output of the producer
    (off the hinge), bn its bnbuf.  dz = gq*[s*y+t>0] is exact: c = 1 for sum dz.  xhat = fma(y, inv, m) with m = -mean*inv
    rounded, within 2u*(|y|+|mean|)*|inv| of (y-mean)*inv: c = 2 for sum dz*xhat with S = sum |dz|*(|y|+|mean|)*|inv|."""
    C_ = gq.shape[-1]
    gq, yin = gq.reshape(-1, C_), yin.reshape(-1, C_)
    bn = bn.double().to(gq.device)
    acc = [torch.zeros(C_, dtype=torch.float64, device=gq.device) for _ in range(4)]
    step = max(1, (8 << 20) // C_)                       # fp64 temporaries of at most 8 M elements
    for m0 in range(0, gq.shape[0], step):
        g, y = gq[m0:m0 + step].double(), yin[m0:m0 + step].double()
        dz = g * relu_mask(y, bn[0], bn[1])
        xhat = (y - bn[5]) * bn[6]
        xabs = (y.abs() + bn[5].abs()) * bn[6].abs()
        for a_, v in zip(acc, (dz, dz.abs(), dz * xhat, dz.abs() * xabs)):
            a_ += v.sum(0)
    P = table.shape[-1]
    p = table.double().sum(-1).to(gq.device)
    a = check_sum_bound(p[0], acc[0], acc[1], M, P, 1, what + " sum dz", None, family)
    b = check_sum_bound(p[1], acc[2], acc[3], M, P, 2, what + " sum dz*xhat", None, family)
    return max(a, b)


def prod_slack(a, b):
    """element-wise slack of a product of two interval operands: |a.mid|*b.half + |b.mid|*a.half + a.half*b.half"""
    return a.mid.abs() * b.half + b.mid.abs() * a.half + a.half * b.half


def pad_hw(x, p):
    """zero-pad an NHWC tensor by p rows / columns on each side"""
    if p == 0:
        return x
    N, H, W, C_ = x.shape
    out = torch.zeros((N, H + 2 * p, W + 2 * p, C_), dtype=x.dtype, device=x.device)
    out[:, p:p + H, p:p + W] = x
    return out


def onload_fwd_terms(a, w, bias=None, stride=1, pad=None, device="cpu"):
    """(ref, slack, S) of check_onload_bound for a forward conv over the interval operand a (N,H,W,Ci), w (Co,Ci,k,k)"""
    aw = _f64(w, device).abs()
    ref = ref_dense_fwd(a.mid, w, bias, stride, pad, device)
    slack = ref_dense_fwd(a.half, aw, None, stride, pad, device)
    S = ref_dense_fwd(a.amax, aw, None if bias is None else bias.abs(), stride, pad, device)
    return ref, slack, S


def onload_dgrad_terms(d, w, H, W, stride=1, pad=None, resid=None, device="cpu"):
    """(ref, slack, S) of check_onload_bound for an input gradient over the interval operand d (N,Ho,Wo,Co), w (Co,Ci,k,k)"""
    aw = _f64(w, device).abs()
    ref = ref_dense_dgrad(d.mid, w, H, W, stride, pad, device)
    slack = ref_dense_dgrad(d.half, aw, H, W, stride, pad, device)
    S = ref_dense_dgrad(d.amax, aw, H, W, stride, pad, device)
    if resid is not None:
        r = _f64(resid, device)
        ref, S = ref + r, S + r.abs()
    return ref, slack, S


def wgrad_terms(a, d, k, stride=1, pad=None, device="cpu"):
    """(ref, S, slack) of check_sum_bound for a dense weight gradient over interval operands a (N,H,W,Ci), d (N,Ho,Wo,Co)
    -> (Co,Ci,k,k).  slack = sum prod_slack = S - sum |a.mid||d.mid|, because amax = |mid| + half for any interval (exactly zero
    for two zero-width intervals: both sums are then the same computation)."""
    ref = ref_dense_wgrad(a.mid, d.mid, k, stride, pad, device)
    S = ref_dense_wgrad(a.amax, d.amax, k, stride, pad, device)
    slack = (S - ref_dense_wgrad(a.mid.abs(), d.mid.abs(), k, stride, pad, device)).clamp_min(0)
    return ref, S, slack


def ref_dw_wgrad_s(x, dy, k, stride=1, device="cpu"):
    """weight gradient of ref_dw_fwd_s: x (N,H,W,C), dy (N,Ho,Wo,C) -> (C,k,k)"""
    x, dy = _f64(x, device), _f64(dy, device)
    N, H, W, C_ = x.shape
    _, Ho, Wo, _ = dy.shape
    xp = pad_hw(x, k // 2)
    dw = torch.zeros((C_, k, k), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            dw[:, kh, kw] = (xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] * dy).sum((0, 1, 2))
    return dw


def ref_dw_dgrad_s(dy, w, H, W, stride=1, device="cpu"):
    """input gradient of ref_dw_fwd_s: dy (N,Ho,Wo,C) -> (N,H,W,C)"""
    dy, w = _f64(dy, device), _f64(w, device)
    N, Ho, Wo, C_ = dy.shape
    k = w.shape[-1]
    p = k // 2
    gp = torch.zeros((N, max(H + 2 * p, (Ho - 1) * stride + k), max(W + 2 * p, (Wo - 1) * stride + k), C_), dtype=torch.float64, device=device)
    for kh in range(k):
        for kw in range(k):
            gp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] += dy * w[:, kh, kw]
    return gp[:, p:p + H, p:p + W].contiguous()


def dw_fwd_terms(a, w, bias=None, stride=1, device="cpu"):
    """(ref, S) of check_dw_bound for the depthwise forward over the fp32 interval operand a = act_interval(..., bf16=False) (or
    Interval.exact of a plain input): ref over the exact operand a.val, S = |bias| + sum a.D*|w|"""
    aw = _f64(w, device).abs()
    ref = ref_dw_fwd_s(a.val, w, bias, stride, device)
    S = ref_dw_fwd_s(a.D, aw, None if bias is None else bias.abs(), stride, device)
    return ref, S


def dw_dgrad_terms(d, w, H, W, stride=1, device="cpu"):
    """(ref, S) of check_dw_bound for the depthwise input gradient over d = dy_interval(..., bf16=False): S = sum D*|w|"""
    aw = _f64(w, device).abs()
    return ref_dw_dgrad_s(d.val, w, H, W, stride, device), ref_dw_dgrad_s(d.D, aw, H, W, stride, device)


def dw_wgrad_terms(a, d, k, stride=1, device="cpu"):
    """(ref, S, slack) of check_sum_bound (c = 2) for the depthwise weight gradient over fp32 interval operands (slack as in
    wgrad_terms)"""
    ref = ref_dw_wgrad_s(a.mid, d.mid, k, stride, device)
    S = ref_dw_wgrad_s(a.amax, d.amax, k, stride, device)
    slack = (S - ref_dw_wgrad_s(a.mid.abs(), d.mid.abs(), k, stride, device)).clamp_min(0)
    return ref, S, slack


# ---- squeeze-excite, stem gradients, glue and the finalizes ------------------------------------------------------------------------
# Same conventions: u = 2^-24, the host brackets the device's fp32 evaluation in fp64 and never re-enacts it, rounding (to fp32 or
# to bf16) is monotone so a stored value lies between the rounded ends of its bracket, sums get check_sum_bound's form.  Two shapes
# of check: an Interval that already holds EVERY rounding up to the stored fp32 value (check_interval), and an Interval of the fp32
# value that is then rounded once to bf16 (check_store_bound).
TINY32 = 2.0 ** -149     # one fp32 denormal step: the absolute floor of a rounding whose result is subnormal
D64 = 2.0 ** -48         # relative allowance for a chain of at most 32 double-precision operations (each 2^-53)


def _widen(lo, hi, n=1):
    """n further fp32 roundings of a value known to lie in [lo, hi]: each moves it by at most u of its own magnitude, so the result
    lies in [lo - f|lo|, hi + f|hi|] with f = (1+u)^n - 1 (a value of the other sign than an end is inside anyway)"""
    f = (1 + U32) ** n - 1
    return lo - f * lo.abs(), hi + f * hi.abs()


def imul(a, b, n=1):
    """Interval of fl(a*b) for a in [a.lo, a.hi], b in [b.lo, b.hi]: hull of the four corner products (a product is monotone in
    each factor), widened by n roundings"""
    al, ah, bl, bh = torch.broadcast_tensors(a.lo, a.hi, b.lo, b.hi)
    c = torch.stack([al * bl, al * bh, ah * bl, ah * bh])
    lo, hi = _widen(c.min(0).values, c.max(0).values, n) if n else (c.min(0).values, c.max(0).values)
    return Interval(lo, hi)


def sigmoid_interval(v, device=None):
    """Bracket of se_sigmoid(v) = 1.f / (1.f + __expf(-v)) (csrc/mnas_se.hip) around the fp64 sigmoid s; v fp32 as the device reads it.
    __expf(x) is the hardware 2^t of t = fl(x * fl(log2 e)).  With e = exp(-v):
      the constant fl(log2 e) and the product each move t by at most u|t|, i.e. 2^t by a factor within 2|t| ln2 u = 2|v| u of 1;
      the hardware exponential is taken at its documented accuracy of one ulp = 2u relative -- the ONE assumption here that IEEE 754
      does not give; the mnas_se_gate sweep of tests/test_gpu_se.py checks it directly;
      the add 1.f + e and the division (IEEE: the build has no fast-math) are within u each;
      an error of e reaches s = 1/(1+e) with the factor e/(1+e) <= 1.
    To first order (2|v| + 4)u; (2|v| + 6)u leaves room for every second-order term at |v| <= 2^10:
        |se_sigmoid(v) - s| <= (2|v| + 6) u s + 2^-126     (the floor: a subnormal quotient, an exponential flushed to zero)
    and the quotient of 1 by a number >= 1 lies in [0, 1]."""
    v = v.double() if device is None else _f64(v, device)
    s = torch.sigmoid(v)
    r = (2 * v.abs() + 6) * U32 * s + 2.0 ** -126
    return Interval((s - r).clamp_min(0.0), (s + r).clamp_max(1.0), s, s)


def check_sigmoid(got, v, what, family="se_sigmoid"):
    """got = se_sigmoid(v) from the device: inside sigmoid_interval(v); returns (and keeps in WORST) the largest
    |got - s| / ((2|v| + 6) u s + 2^-126), the error against the bracket's half width BEFORE its ends are clamped to [0, 1]"""
    iv = sigmoid_interval(v)
    check_interval(got, iv, what, None)
    r = float(((got.double().cpu() - iv.val).abs() / ((2 * v.double().abs() + 6) * U32 * iv.val + 2.0 ** -126)).max())
    if family:
        WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def sig1m_interval(v, device=None):
    """Bracket of fl(sg * fl(1.f - sg)), sg = se_sigmoid(v): g(x) = x(1-x) over the bracket [l, h] of sg -- g rises up to 1/2 and
    falls after it, so its range is [min(g(l), g(h)), max(g(l), g(h))], or up to 1/4 where l <= 1/2 <= h -- widened by the two
    roundings (the subtraction, the product).  Not linearised: 1 - sg cancels for large v, and the bracket of sg is then a large
    share of it."""
    sg = sigmoid_interval(v, device)
    gl, gh = sg.lo * (1 - sg.lo), sg.hi * (1 - sg.hi)
    lo, hi = torch.minimum(gl, gh), torch.maximum(gl, gh)
    hi = torch.where((sg.lo <= 0.5) & (sg.hi >= 0.5), torch.full_like(hi, 0.25), hi)
    lo, hi = _widen(lo, hi, 2)
    return Interval(lo, hi, None, sg.val * (1 - sg.val))


def gate_nhwc(gate, shape):
    """(N, C) gate Interval -> broadcastable against (N, H, W, C)"""
    N, C_ = gate.lo.shape
    view = (N,) + (1,) * (len(shape) - 2) + (C_,)
    return Interval(gate.lo.view(view), gate.hi.view(view), None, None if gate.val is None else gate.val.view(view))


def gated_act_interval(z, s, t, gate, bf16, device="cpu"):
    """Interval of the gated operand fl(a * sg): a = relu(fma(z, s, t)) (s, t None: a = z, exact) and sg the gate of the element's
    (image, channel), an Interval >= 0 (sigmoid_interval) broadcastable against z -- what act8g (MnasConvGemm.gate) and k_se_scale
    form: ONE more fp32 rounding after act_interval's value.  Both factors' brackets are >= 0 under the activation, so the product
    lies in [lo*glo*(1-u), hi*ghi*(1+u)]; a plain (signed) a takes the hull of the corner products.  bf16=True: both ends rounded
    to bf16 (pack8), and at most MAX_ACT_SPLIT of the elements may straddle a rounding boundary, as for act_interval."""
    if s is None:
        a = Interval.exact(z, device)
    else:
        a = act_interval(z, s, t, False, device)
    g = Interval(_f64(gate.lo, device), _f64(gate.hi, device))
    p = imul(a, g, 1)
    lo, hi = p.lo, p.hi
    gv = _f64(gate.val, device) if gate.val is not None else (g.lo + g.hi) / 2
    val = a.val * gv
    if bf16:
        lo, hi = _bf16_64(lo), _bf16_64(hi)
    iv = Interval(lo, hi, a.D * g.hi, val)
    if bf16:
        share = iv.split_share()
        assert share <= MAX_ACT_SPLIT, "gated act operand: %.3g of the bf16 elements straddle a rounding boundary (limit %.3g)" % (share, MAX_ACT_SPLIT)
        Interval.worst_act = max(Interval.worst_act, share)
    return iv


def check_interval(hip, iv, what, family):
    """hip: an fp32 output whose EVERY rounding is already inside iv: lo - 2^-149 <= hip <= hi + 2^-149 for every element (asserted
    on the ends themselves: an output may sit exactly on one).  Returns max |hip - mid| / (half + 2^-149), also kept in WORST."""
    h = hip.double()
    lo, hi = iv.lo.to(h.device), iv.hi.to(h.device)
    assert h.shape == lo.shape, (what, h.shape, lo.shape)
    bad = ~((h >= lo - TINY32) & (h <= hi + TINY32))          # (a NaN fails)
    ratio = (h - (lo + hi) / 2).abs() / ((hi - lo) / 2 + TINY32)
    if bool(bad.any()):
        r = torch.where(bad, ratio, torch.zeros_like(ratio))
        idx = tuple(int(v) for v in torch.unravel_index(r.reshape(-1).argmax(), r.shape)) if r.dim() else ()
        raise AssertionError("%s: %d of %d elements outside the per-element bound; worst at %s: got %r, bracket [%r, %r] (x%.2f)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(h[idx]), float(lo[idx]), float(hi[idx]), float(ratio[idx])))
    worst = min(1.0, float(ratio.max())) if ratio.numel() else 0.0       # (an element exactly on an end: 1 up to the fp64 rounding of mid)
    if family:
        WORST[family] = max(WORST.get(family, 0.0), worst)
    return worst


def check_store_bound(hip, iv, what, family):
    """A bf16 elementwise store (pack8: round to nearest even) of an fp32 value known to lie in iv = [lo, hi]: rounding is monotone,
    so EVERY element lies in [bf16(lo), bf16(hi)] -- asserted as such (it is what rejects a value rounded twice) -- and therefore
    within 2^-8 (|mid| + half) + half of mid, which is what the ratio in WORST is taken against."""
    h = hip.double()
    lo, hi = _bf16_64(iv.lo).to(h.device), _bf16_64(iv.hi).to(h.device)
    assert h.shape == lo.shape, (what, h.shape, lo.shape)
    bad = ~((h >= lo) & (h <= hi))
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside the per-element bound (not in [bf16(lo), bf16(hi)]); first at %s: got %r, bracket [%r, %r]"
                             % (what, int(bad.sum()), bad.numel(), idx, float(h[idx]), float(lo[idx]), float(hi[idx])))
    mid, half = iv.mid.to(h.device), iv.half.to(h.device)
    return _assert_bound(h, mid, 2.0 ** -8 * (mid.abs() + half) + half, what, family)


def sum_bound(S, M, P, c, slack=None):
    """check_sum_bound's bound as a tensor: (c*M + P + 1)*2^-22*S + slack"""
    b = (c * M + P + 1) * 2.0 ** -22 * S.double()
    return b if slack is None else b + slack.double()


def sum_interval(ref, S, M, P, c, slack=None):
    """the fp32 sum of check_sum_bound as an Interval, for a result that is processed further (times a factor, through a relu)"""
    b = sum_bound(S, M, P, c, slack)
    return Interval(ref.double() - b, ref.double() + b)


def se_apply_interval(gq, u, dz, HW, device="cpu"):
    """k_se_bwd_apply's fp32 value fma(gq, sg, zz) per element, gq (N,H,W,C) bf16 values, u, dz (N,C): sg in sigmoid_interval(u);
    zz = fl(dz * fl(1/HW)): the reciprocal within u, the product within u more; the fma rounds the exact gq*sg + zz once, an
    unfused evaluation the product too: within u(|gq| sg + |zz|) either way."""
    gq = _f64(gq, device)
    sg = gate_nhwc(sigmoid_interval(u, device), gq.shape)
    inv = 1.0 / HW
    zz = gate_nhwc(imul(Interval.exact(dz, device), Interval(torch.full((), inv * (1 - U32), dtype=torch.float64, device=device),
                                                             torch.full((), inv * (1 + U32), dtype=torch.float64, device=device)), 1), gq.shape)
    p = imul(Interval.exact(gq), sg, 0)
    r = U32 * (p.amax + zz.amax) * (1 + U32)
    return Interval(p.lo + zz.lo - r, p.hi + zz.hi + r)


def se_reduce_terms(gs, a, HW):
    """(ref, S, slack) per (image, channel) of sum_hw gs*a for mnas_se_bwd_reduce: gs (N,H,W,C) exact bf16 values, a the fp32
    operand Interval (act_interval(..., bf16=False), or Interval.exact for a plain input).  One fma per pixel (c = 1)."""
    g = gs.double().to(a.lo.device)
    N, C_ = g.shape[0], g.shape[-1]
    f = lambda t: t.reshape(N, HW, C_).sum(1)
    return f(g * a.mid), f(g.abs() * a.amax), f(g.abs() * a.half)


def se_geom(N, HW, C_):
    """(G, R, chunk, splits) as csrc/mnas_se.hip::se_geom derives them; the tests assert it against mnas_se_scratch_bytes /
    mnas_se_bwd_apply_cols"""
    G_ = C_ // 8
    R = 256 // G_
    sp = max(1, min(2048 // N, (HW + 4 * R - 1) // (4 * R)))
    chunk = ((HW + sp - 1) // sp + R - 1) // R * R
    return G_, R, chunk, (HW + chunk - 1) // chunk


def se_proj_finalize_intervals(wp, N, kseg, W, u, dW0=None):
    """mnas_se_proj_finalize from the wpartial table the segment-mode mnas_pw_bwd wrote (read BEFORE the finalize: it folds in
    place): wp (N*kseg, Co, Ci) fp32, W (Co, Ci) the fp32 master weight, u (N, Ci).  p[n] = sum_j wp[n*kseg+j] in fp32.
      du[n][c] = fl(fl(acc * sg) * fl(1 - sg)), acc = sum_o fma(W, p, acc): Co*kseg terms, the term p itself rounded (c = 2), the
        256/Ci output-channel groups met in LDS (P); then the sig1m bracket and one more rounding.
      dW[o][c] (+)= sum_n fl(p[n] * sg[n]): N*kseg terms, c = 2, sg's bracket in the slack; the accumulate add is check_sum_bound's +1.
    Returns (du Interval, dW ref, dW S, dW slack, M of dW)."""
    dev = wp.device
    Co, Ci = W.shape
    p = wp.double().view(N, kseg, Co, Ci)
    pa = p.abs().sum(1)
    p = p.sum(1)
    W = _f64(W, dev)
    G_ = 256 // Ci if Ci <= 256 else 0
    acc = sum_interval((W * p).sum(1), (W.abs() * pa).sum(1), Co * kseg, G_, 2)
    du = imul(acc, sig1m_interval(u, dev), 1)
    sg = sigmoid_interval(u, dev)
    sl, sh = sg.lo.view(N, 1, Ci), sg.hi.view(N, 1, Ci)
    ref, S, slack = (p * (sl + sh) / 2).sum(0), (pa * sh).sum(0), (pa * (sh - sl) / 2).sum(0)
    if dW0 is not None:
        ref, S = ref + _f64(dW0, dev), S + _f64(dW0, dev).abs()
    return du, ref, S, slack, N * kseg


def se_fc_fwd_intervals(z, W1, b1, W2, b2):
    """mnas_se_fc_fwd (fp32 dot products, fma or multiply-and-add: c = 2): hb = relu(W1 z + b1) over E terms plus the bias,
    u = W2 hb + b2 over R terms plus the bias with |W2| err(hb) as slack, gate = se_sigmoid(u) over u's bracket (the sigmoid and
    both ends of its bracket rise with v for |v| < 16, asserted).  Returns (hb, u, gate) Intervals (N,R), (N,E), (N,E)."""
    z, W1, b1, W2, b2 = (t.double() for t in (z, W1, b1, W2, b2))
    E, R = W2.shape
    pre = sum_interval(z @ W1.t() + b1, z.abs() @ W1.abs().t() + b1.abs(), E, 1, 2)
    hb = Interval(torch.relu(pre.lo), torch.relu(pre.hi))
    u = sum_interval(hb.mid @ W2.t() + b2, hb.amax @ W2.abs().t() + b2.abs(), R, 1, 2, hb.half @ W2.abs().t())
    assert float(u.amax.max()) < 16
    gate = Interval(sigmoid_interval(u.lo).lo, sigmoid_interval(u.hi).hi)
    return hb, u, gate


def se_fc_bwd_terms(du, z, hb_dev, W1, W2, base=None):
    """mnas_se_fc_bwd against fp64, every product c = 2.  hb_dev: the hidden row the device stored (the mask and dW2's operand are
    the device's own values).  dh = (du W2)[hb_dev > 0]: E terms, 256/(2R) row slices (P); dz = dh W1: R terms over dh's bracket;
    dW1 / db1 / dW2 / db2: N terms in 16 image phases (P = 16), plus the accumulate target `base` (a dict) where given.
    Returns dh, dz Intervals and {name: (ref, S, slack, c)} for check_sum_bound with M = N, P = 16."""
    du, z, hb, W1, W2 = (t.double() for t in (du, z, hb_dev, W1, W2))
    N, E = du.shape
    R = W1.shape[0]
    m = (hb > 0).double()
    dh = sum_interval((du @ W2) * m, (du.abs() @ W2.abs()) * m, E, 256 // (2 * R), 2)
    dz = sum_interval(dh.mid @ W1, dh.amax @ W1.abs(), R, 0, 2, dh.half @ W1.abs())
    t = {"dW1": (dh.mid.t() @ z, dh.amax.t() @ z.abs(), dh.half.t() @ z.abs(), 2),
         "db1": (dh.mid.sum(0), dh.amax.sum(0), dh.half.sum(0), 1),
         "dW2": (du.t() @ hb, du.abs().t() @ hb.abs(), None, 2),
         "db2": (du.sum(0), du.abs().sum(0), None, 1)}
    if base is not None:
        t = {k: (r + base[k].double(), S + base[k].double().abs(), sl, c) for k, (r, S, sl, c) in t.items()}
    return dh, dz, t


def stem_dgrad_terms(d, w, H, W, aff=None, device="cpu"):
    """(ref, bound) of mnas_stem_dgrad's fp32 NCHW result.  d: the bf16 dy Interval (N,Ho,Wo,Co) (dy_interval(..., bf16=True): dy8 and
    pack_bf16 in the kernel); w: the weights AS THE KERNEL ROUNDS THEM, bf16 values (Co,3,3,3).  Every product of two bf16 values is
    exact in fp32 and every term one fmaf: at most K = 4*Co roundings (four contributing output pixels at most) of 2^-24 of a
    running magnitude <= S = sum |dy||w|, doubled as in check_gemm_bound: (K+1)*2^-23*S, plus the slack of the dy brackets.  No bf16
    store.  in_affine: one more product, acc * scale[plane]: the bound times |scale| and u of the scaled result more."""
    aw = _f64(w, device).abs()
    Co = w.shape[0]
    ref = ref_dense_dgrad(d.mid, w, H, W, 2, 1, device)
    slack = ref_dense_dgrad(d.half, aw, H, W, 2, 1, device)
    S = ref_dense_dgrad(d.amax, aw, H, W, 2, 1, device)
    bound = (4 * Co + 1) * 2.0 ** -23 * S + slack
    if aff is not None:
        sc = _f64(aff[0], device)
        ref, bound = ref * sc, bound * sc.abs()
        bound = bound + U32 * (ref.abs() + bound)
    return ref.permute(0, 3, 1, 2).contiguous(), bound.permute(0, 3, 1, 2).contiguous()


def stem_wgrad_band_rows(W, Wo):
    """output rows per band of k_stem_wgrad: 4, halved while stem_lds (csrc/mnas_stem.hip) exceeds 52 KB"""
    def lds(rb):
        lw = (W + 4 + 1) & ~1
        return 3 * (2 * rb + 1) * lw * 2 + 5 * 32 * 4 + ((rb * Wo + 31) & ~31) * 40 * 2
    rb = 4
    while rb > 1 and lds(rb) > 52 * 1024:
        rb >>= 1
    return rb


def pool_act_terms(a, HW):
    """(ref, bound) of mnas_pool_act: a the fp32 operand Interval (N,HW,C) (act_interval(..., bf16=False) or Interval.exact).  The
    sum of HW terms over R row lanes is check_sum_bound's (c = 1: one add per term; the fma of a virtual operand is in the
    bracket, whose half width is the slack); the division by (float)HW (exact for HW < 2^24, IEEE) rounds once more."""
    C_ = a.lo.shape[-1]
    R = 256 // (C_ // 8)
    b = sum_bound(a.amax.sum(1), HW, R, 1, a.half.sum(1))
    ref = a.mid.sum(1)
    return ref / HW, b / HW + U32 * (ref.abs() + b) / HW


def add_act_interval(A, B=None):
    """fp32 value of mnas_add_act per element: act(a) [+ act(b)] from the operands' fp32 Intervals; the add rounds once more"""
    if B is None:
        return A
    lo, hi = _widen(A.lo + B.lo, A.hi + B.hi, 1)
    return Interval(lo, hi)


def partial_sum_interval(p):
    """bn_partial_sums<TPC> (csrc/mnas_elementwise.hip) over the last dimension of the fp32 table p: thread t of TPC (64 up to 256
    partials, 256 above) adds the partials t + 4*TPC*i + TPC*j into fp32 accumulator j, T = ceil(nparts / (4*TPC)) of them each,
    the first onto 0.f: T - 1 roundings of at most u of the accumulator's running magnitude, together (T-1)*u*sum|p| -- zero up to
    256 partials and again from 257 to 1024.  Everything after that is double: D64 of sum|p|."""
    n = p.shape[-1]
    tpc = 64 if n <= 256 else 256
    T = -(-n // (4 * tpc))
    s, a = p.double().sum(-1), p.double().abs().sum(-1)
    d = ((T - 1) * U32 + D64) * a
    return Interval(s - d, s + d)


def _f32_store(lo, hi, mag=None):
    """a double result in [lo, hi] (computed with double error D64 of `mag`, default its own magnitude) stored as fp32"""
    m = torch.maximum(lo.abs(), hi.abs()) if mag is None else mag
    lo, hi = lo - D64 * m, hi + D64 * m
    lo, hi = _widen(lo, hi, 1)
    return Interval(lo, hi)


def _hull(*ts):
    c = torch.stack(torch.broadcast_tensors(*ts))
    return c.min(0).values, c.max(0).values


def bn_fwd_finalize_intervals(partial, count, gamma, beta, rm, rv, momentum, eps):
    """mnas_bn_fwd_finalize (training) from the fp32 table partial [2][C][nparts] exactly as given to the kernel; gamma, beta, rm, rv
    fp32 [C]; momentum, eps as the fp32 values the ABI passes.  Bracketed, not linearised (var = s2/count - mean^2 cancels):
      s1, s2 in partial_sum_interval; mean = s1/count; var = s2/count - mean^2 within ds2/count + 2|mean| dmean + dmean^2 (and D64
      of s2/count + mean^2: the double subtraction cancels too), clamped at 0 at both ends as the kernel clamps;
      invstd = 1/sqrt(var + eps) falls with var; s = gamma invstd, t = beta - mean gamma invstd, running_mean, running_var
      (unbiased: var count/(count-1), var itself at count <= 1) are (bi)linear in (mean, invstd) resp. var: the hull over the corners.
    Each output is then rounded once to fp32.  Returns {name: Interval} for s, t, mean, invstd, running_mean, running_var."""
    s1, s2 = partial_sum_interval(partial[0]), partial_sum_interval(partial[1])
    g, b, rm, rv = gamma.double(), beta.double(), rm.double(), rv.double()
    mom, eps = float(torch.tensor(momentum, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    ml, mh = s1.lo / count, s1.hi / count
    mean, dmean = (ml + mh) / 2, (mh - ml) / 2
    e2 = s2.mid / count
    var = e2 - mean * mean
    dvar = s2.half / count + 2 * mean.abs() * dmean + dmean * dmean + D64 * (e2.abs() + mean * mean)
    vl, vh = (var - dvar).clamp_min(0.0), (var + dvar).clamp_min(0.0)
    il, ih = 1 / torch.sqrt(vh + eps), 1 / torch.sqrt(vl + eps)
    unb = count / (count - 1.0) if count > 1.0 else 1.0
    out = {"mean": _f32_store(ml, mh), "invstd": _f32_store(il, ih)}
    out["s"] = _f32_store(*_hull(g * il, g * ih))
    tl, th = _hull(*[b - m_ * g * i_ for m_ in (ml, mh) for i_ in (il, ih)])
    out["t"] = _f32_store(tl, th, b.abs() + torch.maximum(ml.abs(), mh.abs()) * g.abs() * ih)
    out["running_mean"] = _f32_store(*_hull((1 - mom) * rm + mom * ml, (1 - mom) * rm + mom * mh), (1 - mom) * rm.abs() + mom * torch.maximum(ml.abs(), mh.abs()))
    out["running_var"] = _f32_store((1 - mom) * rv + mom * vl * unb, (1 - mom) * rv + mom * vh * unb)
    return out


def bn_bwd_finalize_intervals(partial, count, bn, dgamma0=None, dbeta0=None, frozen=False, dbias0=None):
    """mnas_bn_bwd_finalize / _frozen from the fp32 table partial [2][C][nparts] (sum dz, sum dz*xhat) and the bnbuf rows s (0),
    mean (5), invstd (6) as given: s1, s2 in partial_sum_interval, then double, one fp32 rounding per output.
      rows 2..4: c1 = s; c2 = -s invstd s2/count; c3 = s (mean invstd s2/count - s1/count): hull over the ends of s1, s2;
      dgamma = dgamma0 + fl(s2), dbeta = dbeta0 + fl(s1) (accumulate: one more fp32 add); frozen: dbias = dbias0 + fl(s s1), rows 2..4 untouched."""
    s1, s2 = partial_sum_interval(partial[0]), partial_sum_interval(partial[1])
    bn = bn.double()
    s, mean, inv = bn[0], bn[5], bn[6]

    def acc(iv, base):
        if base is None:
            return iv
        lo, hi = _widen(iv.lo + base.double(), iv.hi + base.double(), 1)
        return Interval(lo, hi)
    out = {"dgamma": acc(_f32_store(s2.lo, s2.hi), dgamma0), "dbeta": acc(_f32_store(s1.lo, s1.hi), dbeta0)}
    if frozen:
        out["dbias"] = acc(_f32_store(*_hull(s * s1.lo, s * s1.hi)), dbias0)
        return out
    out["c1"] = Interval(s, s)
    out["c2"] = _f32_store(*_hull(-s * inv * s2.lo / count, -s * inv * s2.hi / count))
    c3 = [s * (mean * inv * b_ / count - a_ / count) for a_ in (s1.lo, s1.hi) for b_ in (s2.lo, s2.hi)]
    out["c3"] = _f32_store(*_hull(*c3), s.abs() * ((mean * inv).abs() * s2.amax + s1.amax) / count)
    return out


def bn_fwd_partials(u, count):
    """The fp32 table [2][C+3][nparts] of the mnas_bn_fwd_finalize tests from u = uniform(-1, 1) of that shape, built in fp64 and
    rounded ONCE to fp32.  Channels [0, C): mean ~ 0.3*u, var in [0.5, 0.9] (the distribution the test always had).  The last
    three: |mean|/std = 30 (mean 60, var 4), |mean|/std = 300 (mean 600, var 4) -- where var = s2/count - mean^2 cancels 3 resp. 5
    decimal digits -- and a constant channel (every element 1.5) whose sum of squares is rounded DOWN by 2^-20, so that var comes
    out negative and takes the clamp."""
    u = u.double()
    nparts = u.shape[-1]
    per = count / nparts
    mean_p = 0.3 * u[0]
    p = torch.stack([per * mean_p, per * (mean_p ** 2 + 0.5 + 0.4 * u[1].abs())])
    for ch, m in ((-3, 60.0), (-2, 600.0)):
        p[0, ch] = per * m * (1 + 0.01 * u[0, ch])
        p[0, ch] = p[0, ch].float().double()
        m_act = p[0, ch].sum() / count                        # the mean the table really holds
        p[1, ch] = per * (m_act ** 2 + 4.0) * (1 + 0.01 * (u[1, ch] - u[1, ch].mean()))
    p[0, -1] = per * 1.5
    p[1, -1] = per * 2.25 * (1 - 2.0 ** -20)
    return p.float()


def gated_fwd_inputs(shape, O):
    """(y NCHW, s, t, u, w, bias) of tests/test_gpu_se.py::test_gated_project_forward (also read by the CPU test of the gated
    operand's straddle share)"""
    N, H, W, Ci, Co = shape
    y = bf16r(O.det_uniform((N, Ci, H, W), 810))
    s, t = 1 + 0.3 * O.det_uniform((Ci,), 811), 0.2 * O.det_uniform((Ci,), 812)
    u = 2.0 * O.det_uniform((N, Ci), 813)
    w = bf16r(O.det_param("g.conv.weight", (Co, Ci, 1, 1), 3))
    bias = O.det_uniform((Co,), 814) * 0.1
    return y, s, t, u, w, bias


# ---- the fp32 tail of the step: classifier-head GEMMs, cross-entropy, flat-buffer optimizers ----------------------------------------
# Same conventions.  The references are fp64 arithmetic on the fp32 values the device reads; host-side scalars (drop_scale, Adam's
# bias corrections, lr / bc1) are reproduced bit for bit in float32 and enter as exact data.
def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _pow2(n, seed, lo, hi):
    """n exact powers of two 2^k, k uniform in [lo, hi]"""
    k = torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed))
    return torch.pow(torch.tensor(2.0), k.float())


def f32(v):
    """a Python float holding the fp32 value the C ABI passes for v"""
    return float(torch.tensor(v, dtype=torch.float32))


def _w32(lo, hi, n=1):
    """_widen plus the absolute floor of n roundings whose result is subnormal"""
    lo, hi = _widen(lo, hi, n)
    return lo - n * TINY32, hi + n * TINY32


def _iv(x, like=None):
    """a float scalar or a tensor -> exact Interval (on `like`'s device)"""
    if not torch.is_tensor(x):
        x = torch.tensor(x, dtype=torch.float64, device=None if like is None else like.device)
    x = x.double()
    return Interval(x, x)


def iadd(a, b, n=1, sign=1.0):
    """Interval of fl(a + sign*b): the exact sum of the ends, widened by n roundings"""
    lo, hi = (a.lo + b.lo, a.hi + b.hi) if sign > 0 else (a.lo - b.hi, a.hi - b.lo)
    lo, hi = _w32(lo, hi, n) if n else (lo, hi)
    return Interval(lo, hi)


def idiv(a, b, n=1, ulps=1):
    """Interval of fl(a / b), b of one sign and never zero: hull of the corner quotients, n roundings of ulps * u each"""
    assert bool(((b.lo > 0) | (b.hi < 0)).all())
    c = torch.stack(torch.broadcast_tensors(a.lo / b.lo, a.lo / b.hi, a.hi / b.lo, a.hi / b.hi))
    lo, hi = c.min(0).values, c.max(0).values
    f = (1 + ulps * U32) ** n - 1 + D64
    return Interval(lo - f * lo.abs() - n * TINY32, hi + f * hi.abs() + n * TINY32)


def isqrt(a):
    """Interval of sqrtf(a) (IEEE: correctly rounded, monotone); a negative lower end of a bracket of a non-negative value is 0"""
    lo, hi = _w32(torch.sqrt(a.lo.clamp_min(0.0)) * (1 - D64), torch.sqrt(a.hi.clamp_min(0.0)) * (1 + D64), 1)
    return Interval(lo.clamp_min(0.0), hi)


def ifma(s, a, c):
    """Interval of fmaf(s, a, c): the exact product plus c, rounded once"""
    return iadd(imul(s, a, 0), c, 1)


def check_iv(hip, iv, what, family):
    """check_interval that also takes brackets with an infinite end: where lo == hi == +-inf the output must equal it"""
    h = hip.double()
    lo, hi = iv.lo.to(h.device), iv.hi.to(h.device)
    inf = torch.isinf(lo) & (lo == hi)
    if bool(inf.any()):
        assert bool((h[inf] == lo[inf]).all()), "%s: outside the per-element bound (an infinite result expected)" % what
        if bool(inf.all()):
            return 0.0
        return check_interval(hip[~inf], Interval(lo[~inf], hi[~inf]), what, family)
    return check_interval(hip, iv, what, family)


# ---- classifier-head GEMMs (csrc/mnas_head.hip: k_head_gemm) -------------------------------------------------------------------------
HEAD_SIZES = [(256, 320, 512), (37, 320, 1000), (5, 512, 10), (64, 256, 1000), (130, 70, 65),
              (1, 1, 1), (1, 129, 1), (33, 128, 33), (32, 127, 32)]
HEAD_PS = [0.0, 0.5, 0.2, 0.999]


def head_chain(K):
    """fmaf per output and wave: every K step of 128 gives each of the 8 waves 16 k, zero-padded steps included"""
    return 16 * -(-K // 128)


def head_drop_scale(p):
    """head_drop: (float)(1.0 / (1.0 - (double)p)) of the fp32 p the ABI passes"""
    return float(torch.tensor(1.0 / (1.0 - f32(p)), dtype=torch.float64).float())


def head_dropped(x, keep, p):
    """the operand under dropout as k_head_gemm stages it: the single fp32 product x * drop_scale (stored to LDS before any
    FMA, so nothing contracts into it) where kept, 0 elsewhere -- reproduced bit for bit by a float32 multiply"""
    if p == 0:
        return x.clone()
    sc = torch.tensor(head_drop_scale(p), dtype=torch.float32)
    return torch.where(keep, x * sc, torch.zeros_like(x))


def head_gemm_interval(A, B, bias=None, C0=None, relu=False, post=None, mask=None):
    """Bracket of one k_head_gemm output tile set: A (M, K), B (K, N) the fp32 operands AS STAGED (head_dropped applied), bias [N],
    C0 the accumulate target, post (M, N) the exact epilogue factor keep * drop_scale of drop_where == 3, mask the exact 0/1
    ReLU mask of bwd_x.  Roundings on the way of any term to the stored value, each at most u of a running magnitude <= S:
      L = 16 * ceil(K / 128) fmaf of the wave's chain (head_chain), 7 adds of the eight partial tiles in wave order (the first, to
      0.f, is exact), the bias add, the drop_where == 3 multiply, the accumulate add: L + 10 counting the exact first add;
      ReLU and mask are exact.  ref = A B + bias (times post) + C0 in fp64, S the same over absolute values; doubled as in
      check_gemm_bound (it absorbs every second-order term):   |hip - ref| <= (L + 10) * 2^-23 * S   for EVERY element.
    The ReLU is monotone: it is applied to the bracket's two ends, no element is excluded; a masked element is exactly 0."""
    A, B = A.double(), B.double()
    K = A.shape[1]
    ref, S = A @ B, A.abs() @ B.abs()
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if post is not None:
        ref, S = ref * post.double(), S * post.double().abs()
    if C0 is not None:
        ref, S = ref + C0.double(), S + C0.double().abs()
    b = (head_chain(K) + 10) * 2.0 ** -23 * S
    lo, hi = ref - b, ref + b
    if relu:
        lo, hi = torch.relu(lo), torch.relu(hi)
    if mask is not None:
        lo, hi = lo * mask.double(), hi * mask.double()
    return Interval(lo, hi)


def head_rowsum_interval(A, r0=None):
    """Bracket of rowsum[m] (+)= sum_k A(m, k) (db of bwd_w): per wave and K step `asum += (a0 + a1) + (a2 + a3)` for each of its
    four groups of four k -- a term passes 2 roundings inside its group and at most 4 * ceil(K / 128) adds of the running sum --,
    then 7 adds of the eight waves' sums (first exact) and the accumulate add: (4 * ceil(K / 128) + 10) roundings, doubled:
        |hip - ref| <= (4 * ceil(K / 128) + 10) * 2^-23 * S,   S = sum_k |A(m, k)| + |r0|."""
    A = A.double()
    ref, S = A.sum(1), A.abs().sum(1)
    if r0 is not None:
        ref, S = ref + r0.double(), S + r0.double().abs()
    b = (4 * -(-A.shape[1] // 128) + 10) * 2.0 ** -23 * S
    return Interval(ref - b, ref + b)


def head_inputs(N, I, O_, scaled, seed=0):
    """(x, w, b, dz, u_prev, c0w, c0b) of the head GEMM bound tests (also read by tests/test_bounds_cpu.py).  scaled: rows and
    columns of every operand times exact powers of two 2^-12 .. 2^12 (a scale per batch row, per input and per output feature;
    w carries out / in, so that no product of the reduction cancels a scale), most outputs then lie far below the tensor's maximum;
    u_prev (the ReLU mask source) holds exact +0.0, -0.0 and the smallest positive subnormal."""
    x, w, b = _rand((N, I), seed + 1), _rand((O_, I), seed + 2) * 0.1, _rand((O_,), seed + 3)
    dz, u_prev = _rand((N, O_), seed + 4), _rand((N, I), seed + 5)
    c0w, c0b = _rand((O_, I), seed + 6) * 0.25, _rand((O_,), seed + 7) * 0.5
    if scaled:
        rn, ri, ro = _pow2(N, seed + 8, -12, 12), _pow2(I, seed + 9, -12, 12), _pow2(O_, seed + 10, -12, 12)
        x, w, b, dz = x * rn[:, None] * ri, w * ro[:, None] / ri, b * ro, dz * rn[:, None] * ro
        c0w, c0b = c0w * ro[:, None] * ri, c0b * ro
    flat = u_prev.view(-1)
    flat[0::7] = 0.0
    flat[1::7] = -0.0
    flat[2::7] = 2.0 ** -149
    return x, w, b, dz, u_prev, c0w, c0b


HEAD_LIVE_K = lambda K: sorted({k for k in (0, 15, 16, 127, 128, K - 1) if 0 <= k < K})
HEAD_PROBE_RC = lambda M: sorted({r for r in (0, 31, 32, M - 1) if 0 <= r < M})


def head_sparse(t, dim, K):
    """t with everything zero along `dim` except the live k"""
    out = torch.zeros_like(t)
    idx = torch.tensor(HEAD_LIVE_K(K))
    out.index_copy_(dim, idx, t.index_select(dim, idx))
    return out


def head_probe_visible(A, B, iv, what):
    """each live term's contribution |A(m,k) B(k,n)| exceeds twice the bound at some probed (row, column)"""
    A, B = A.double(), B.double()
    rows, cols = torch.tensor(HEAD_PROBE_RC(A.shape[0])), torch.tensor(HEAD_PROBE_RC(B.shape[1]))
    half = iv.half.cpu()[rows][:, cols]
    for k in HEAD_LIVE_K(A.shape[1]):
        term = (A[rows, k].abs()[:, None] * B[k, cols].abs()[None, :])
        assert bool((term > 2 * half).any()), "%s: live k = %d would not be seen" % (what, k)


# ---- cross-entropy, plain and soft (k_head_ce, k_head_ce_soft, the mean stages) -------------------------------------------------------
CE_SIZES = [(1, 1), (33, 1), (1, 1000), (7, 255), (7, 256), (7, 513), (257, 10), (600, 257)]
CE_ROWS = ["uniform4", "uniform40", "peak_on", "peak_off", "equal", "plus1000", "minus1000", "neg_inf"]
CE_IGNORE = ["none", "third", "all_but_one", "all"]


def ce_targets(N, Cn):
    i = torch.arange(N)
    return (i * 7 + 3) % Cn, (i * 5 + 1) % Cn


def ce_logits(kind, N, Cn, seed=11):
    """the logit rows of the cross-entropy bound tests; labels are ce_targets' (neg_inf spares both)"""
    u = _rand((N, Cn), seed)
    a, b = ce_targets(N, Cn)
    if kind == "uniform4":
        return u * 4
    if kind == "uniform40":
        return u * 40
    if kind in ("peak_on", "peak_off"):
        z = u.clone()
        at = a if kind == "peak_on" else (a + 1) % Cn
        z[torch.arange(N), at] += 30.0
        return z
    if kind == "equal":
        return torch.full((N, Cn), 0.75)
    if kind == "plus1000":
        return u * 4 + 1000.0
    if kind == "minus1000":
        return u * 4 - 1000.0
    assert kind == "neg_inf"
    z = u * 4
    m = (torch.arange(Cn)[None, :] + torch.arange(N)[:, None]) % 3 == 0
    m[torch.arange(N), a] = False
    m[torch.arange(N), b] = False
    z[m] = float("-inf")
    return z


def ce_ignore(t, how, ignore_index=-100):
    t = t.clone()
    if how == "third":
        t[::3] = ignore_index
    elif how == "all_but_one":
        kept = int(t[t.numel() // 2])
        t[:] = ignore_index
        t[t.numel() // 2] = kept
    elif how == "all":
        t[:] = ignore_index
    return t


def ce_intervals(x, ta, tb=None, lam=None, eps=None, ignore_index=-100):
    """Brackets of dlogits (N, C) and loss_rows (N,) of k_head_ce (eps None) / k_head_ce_soft, by interval propagation through
    the kernel's operations in their UNCONTRACTED form.  csrc/mnas_head.hip is built with -ffp-contract=fast and without any
    fast-math flag: a contracted form (p - q as one fma of e and rse, the loss row's products folded into its sums) rounds less
    often and lies inside the bracket of the uncontracted one.  x fp32 as the device reads it; every operation one rounding (u):
      mx = max_c x (exact); d = fl(x - mx); e = expf(d); se = sum_c e in ceil(C/256) + 9 adds of non-negative terms (the lane's
      strided sum, six butterfly levels, three adds of the four waves): relative (1 + u)^n; rse = 1/se; p = fl(e rse);
      plain: q = [c == t]; soft: wa = fl(1-eps) or fl(fl(1-eps) lam), wb = 0 or fl(fl(1-eps) - wa) (bracketed, so that the fma
      a compiler may form of it is inside), uq = eps/C, q = fl((qa + qb) + uq) -- the first add always has a zero operand --;
      dlogits = fl(fl(p - q) inv), inv = 1/count, count (rows not ignored) exact.
      loss row, plain: fl(fl(logf(se) + mx) - x[t]); soft: lse = fl(logf(se) + mx), fl(fl(fl(wa fl(lse - x[a])) + fl(wb fl(lse -
      x[b]))) + fl(eps fl(lse - fl(sz/C)))) with sz = sum_c x in the same ceil(C/256) + 9 adds (signed terms: absolute
      ((1 + u)^n - 1) sum|x|); with eps == 0 the smoothing term is left out (the kernel multiplies 0 by 0).
    expf, logf and the three divisions are taken at ONE ULP (2u relative): HIP's documented accuracy of these OCML functions,
    the one assumption here that IEEE 754 does not give; an exponential below 2^-126 may come out as zero (+-2^-126).  The tests
    print the measured error / bracket ratio, which is the check of that assumption.  A -inf logit has e = 0 exactly; with
    eps > 0 it makes the row's loss +inf (the smoothing term reads every class).  Ignored and refused rows: dlogits exactly 0;
    loss row 0 resp. NaN (`nan_rows`).  -> dict(dl=Interval, rows=Interval over all rows (0 at invalid ones), valid, nan_rows,
    count)."""
    x = x.double()
    N, Cn = x.shape
    dev = x.device
    ta = ta.to(dev)
    b = ta if tb is None else tb.to(dev)
    l32 = torch.ones(N, dtype=torch.float32, device=dev) if (tb is None or lam is None) else lam.to(dev).float()
    ignored = (ta == ignore_index) | (b == ignore_index)
    inrange = (ta >= 0) & (ta < Cn) & (b >= 0) & (b < Cn) & (l32 >= 0) & (l32 <= 1)
    valid = ~ignored & inrange
    count = int((~ignored).sum())
    a0, b0 = torch.where(valid, ta, torch.zeros_like(ta)), torch.where(valid, b, torch.zeros_like(b))
    rowi = torch.arange(N, device=dev)
    neg = torch.isinf(x) & (x < 0)
    mx = x.max(1, keepdim=True).values
    dlo, dhi = _w32(torch.where(neg, mx, x) - mx, torch.where(neg, mx, x) - mx, 1)
    elo = (torch.exp(dlo) * (1 - 2 * U32 - D64) - 2.0 ** -126).clamp_min(0.0)
    ehi = torch.exp(dhi) * (1 + 2 * U32 + D64) + 2.0 ** -126
    elo, ehi = torch.where(neg, torch.zeros_like(elo), elo), torch.where(neg, torch.zeros_like(ehi), ehi)
    nadd = -(-Cn // 256) + 9
    se = Interval(*_widen(elo.sum(1, keepdim=True), ehi.sum(1, keepdim=True), nadd))
    one = _iv(1.0, x)
    rse = idiv(one, se, 1, 2)
    p = imul(Interval(elo, ehi), rse, 1)
    inv = idiv(one, _iv(float(max(count, 1)), x), 1, 2)
    # the target row q
    if eps is None:
        e32, ome = 0.0, 1.0
        wa = _iv(torch.ones(N, dtype=torch.float64, device=dev))
        wb = _iv(torch.zeros(N, dtype=torch.float64, device=dev))
        same = torch.ones(N, dtype=torch.bool, device=dev)
    else:
        e32 = f32(eps)
        ome = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(e32, dtype=torch.float32))
        same = ta == b
        wa_m = imul(_iv(ome, x), _iv(l32.double()), 1)
        wb_m = iadd(_iv(ome, x), wa_m, 1, -1.0)
        full, zero = torch.full((N,), ome, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
        wa = Interval(torch.where(same, full, wa_m.lo), torch.where(same, full, wa_m.hi))
        wb = Interval(torch.where(same, zero, wb_m.lo), torch.where(same, zero, wb_m.hi))
    qlo, qhi = torch.zeros_like(x), torch.zeros_like(x)
    qlo[rowi, a0], qhi[rowi, a0] = wa.lo, wa.hi
    ns = ~same
    qlo[rowi[ns], b0[ns]], qhi[rowi[ns], b0[ns]] = wb.lo[ns], wb.hi[ns]
    q = Interval(qlo, qhi)
    if e32 != 0.0:
        q = iadd(q, idiv(_iv(e32, x), _iv(float(Cn), x), 1, 2), 1)
    dl = imul(iadd(p, q, 1, -1.0), inv, 1)
    vm = valid[:, None].double() if count > 0 else torch.zeros((N, 1), dtype=torch.float64, device=dev)
    dl = Interval(dl.lo * vm, dl.hi * vm)
    # the loss row
    lg_lo, lg_hi = torch.log(se.lo), torch.log(se.hi)
    f = 2 * U32 + D64
    lg = Interval(lg_lo - f * lg_lo.abs() - D64, lg_hi + f * lg_hi.abs() + D64)
    lse = iadd(lg, _iv(mx), 1)
    lse = Interval(lse.lo[:, 0], lse.hi[:, 0])
    zero_n = torch.zeros(N, dtype=torch.float64, device=dev)
    za, zb = _iv(torch.where(valid, x[rowi, a0], zero_n)), _iv(torch.where(valid, x[rowi, b0], zero_n))
    if eps is None:
        rows = iadd(lse, za, 1, -1.0)
    else:
        m1 = imul(wa, iadd(lse, za, 1, -1.0), 1)
        m2 = imul(wb, iadd(lse, zb, 1, -1.0), 1)
        rows = iadd(m1, m2, 1)
        if e32 != 0.0:
            xf = torch.where(neg, torch.zeros_like(x), x)
            s, sa = xf.sum(1), xf.abs().sum(1)
            fs = (1 + U32) ** nadd - 1
            szc = idiv(Interval(s - fs * sa, s + fs * sa), _iv(float(Cn), x), 1, 2)
            rows = iadd(rows, imul(_iv(e32, x), iadd(lse, szc, 1, -1.0), 1), 1)
            anyneg = neg.any(1)
            inf = torch.full((N,), float("inf"), dtype=torch.float64, device=dev)
            rows = Interval(torch.where(anyneg, inf, rows.lo), torch.where(anyneg, inf, rows.hi))
    z = torch.zeros(N, dtype=torch.float64, device=dev)
    rows = Interval(torch.where(valid, rows.lo, z), torch.where(valid, rows.hi, z))
    return dict(dl=dl, rows=rows, valid=valid, nan_rows=~ignored & ~inrange, count=count)


def ce_mean_interval(rows_dev, count):
    """k_head_loss_mean(_soft) from the loss_rows the device stored (exact data; ignored rows hold 0): the lane's strided sum,
    the butterfly and the four waves are ceil(N/256) + 9 adds -- within ((1 + u)^n - 1) sum|rows| of the exact sum --, then one
    division (one ulp) by the count, which is an exact integer in fp32.  count == 0: 0/0, NaN (returns None)."""
    if count == 0:
        return None
    r = rows_dev.double()
    n = -(-r.numel() // 256) + 9
    s, sa = r.sum(), r.abs().sum()
    f = (1 + U32) ** n - 1
    return idiv(Interval(s - f * sa, s + f * sa), _iv(float(count), r), 1, 2)


def check_ce_mean(loss, rows_dev, count, what, family):
    """the mean against ce_mean_interval; no row counted: NaN; a +inf row (a -inf logit under smoothing): +inf; a NaN row (a
    refused label): NaN"""
    loss = loss.detach().double().cpu().reshape(())
    r = rows_dev.detach().double().cpu()
    if count == 0 or bool(torch.isnan(r).any()):
        assert bool(torch.isnan(loss)), "%s: outside the per-element bound (NaN expected, got %r)" % (what, float(loss))
        return 0.0
    if not bool(torch.isfinite(r).all()):
        assert float(loss) == float(r.sum()), "%s: outside the per-element bound (%r expected, got %r)" % (what, float(r.sum()), float(loss))
        return 0.0
    return check_interval(loss, ce_mean_interval(r, count), what, family)


# ---- flat-buffer optimizers (csrc/mnas_elementwise.hip: k_adam, k_rmsprop, k_sgd and the _ex variants) ---------------------------------
OPT_SIZES = [1, 255, 257, 10007, 2048 * 256 + 300]
OPT_GRID_CAP = 2048 * 256          # opt_blocks: at most 2048 workgroups of 256 lanes; beyond it a lane takes a second trip


def opt_data(n, seed=0):
    """(p, g, m, v, buf) fp32: p, g with per-element power-of-two scales 2^-20 .. 2^4, both signs and exact zeros; m, buf
    non-zero of either sign; v > 0 except: every 11th element has v = 0 AND g = 0 (denom = eps), every 13th a tiny v = 1e-30"""
    p = _rand((n,), seed + 1) * _pow2(n, seed + 2, -20, 4)
    g = _rand((n,), seed + 3) * _pow2(n, seed + 4, -20, 4)
    m = _rand((n,), seed + 5) * 0.1 + 0.01
    buf = _rand((n,), seed + 6) * 0.1 - 0.01
    v = _rand((n,), seed + 7).abs() * 1e-2 + 1e-6
    p[3::17] = 0.0
    g[5::19] = 0.0
    v[7::13] = 1e-30
    v[0::11] = 0.0
    g[0::11] = 0.0
    return p, g, m, v, buf


def adam_bias(b1, b2, step):
    """(bc1, sqrtf(bc2)) as mnas_adam_step forms them: 1.f - powf(beta, (float)step) with the C library's powf (numpy's float32
    power may take another route), a float32 square root"""
    import ctypes
    import ctypes.util
    import numpy as np
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    one = np.float32(1.0)
    bc1 = one - np.float32(libm.powf(ctypes.c_float(b1), ctypes.c_float(float(step))))
    bc2 = one - np.float32(libm.powf(ctypes.c_float(b2), ctypes.c_float(float(step))))
    return float(bc1), float(np.sqrt(bc2, dtype=np.float32))


def _om(v):
    """fl(1.f - v) of the fp32 v"""
    return float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(v, dtype=torch.float32))


def _opt_grad(p, g, wd, gscale, coef):
    """gi = fl(g gscale), _ex: fl(gi coef) (coef an Interval or None), wd != 0: fmaf(wd, p, gi)"""
    gi = imul(_iv(g), _iv(f32(gscale), g), 1)
    if coef is not None:
        gi = imul(gi, coef, 1)
    if f32(wd) != 0.0:
        gi = ifma(_iv(f32(wd), g), _iv(p), gi)
    return gi


def adam_intervals(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, coef=None):
    """Brackets of k_adam's (p, m, v) after ONE launch from the given state, one fp32 rounding per operation of the source in its
    uncontracted form (a contracted `pi - (lr/bc1) (mi/denom)` rounds once less and lies inside): gi as _opt_grad;
    mi = fmaf(b1, m, fl(fl(1-b1) gi)); vi = fmaf(b2, v, fl(fl(fl(1-b2) gi) gi)); denom = fl(fl(sqrtf(vi) / bc2_sqrt) + eps);
    p = fl(pi - fl(fl(lr/bc1) fl(mi / denom))).  sqrtf and / are IEEE (correctly rounded, monotone: no fast-math in the build);
    bc1, bc2_sqrt, lr/bc1, 1-b1, 1-b2 are the host's / the kernel's own fp32 scalars, bit for bit.  The brackets of mi and denom
    are propagated as if independent (a superset)."""
    b1, b2, eps, lr = f32(b1), f32(b2), f32(eps), f32(lr)
    bc1, bc2s = adam_bias(b1, b2, step)
    step_size = float(torch.tensor(lr, dtype=torch.float32) / torch.tensor(bc1, dtype=torch.float32))
    s = lambda c: _iv(c, g)
    gi = _opt_grad(p, g, wd, gscale, coef)
    mi = ifma(s(b1), _iv(m), imul(s(_om(b1)), gi, 1))
    vi = ifma(s(b2), _iv(v), imul(imul(s(_om(b2)), gi, 1), gi, 1))
    vi = Interval(vi.lo.clamp_min(0.0), vi.hi)
    den = iadd(idiv(isqrt(vi), s(bc2s), 1), s(eps), 1)
    pn = iadd(_iv(p), imul(s(step_size), idiv(mi, den, 1), 1), 1, -1.0)
    return dict(p=pn, m=mi, v=vi)


def rmsprop_intervals(p, g, sq, buf, lr, alpha, eps, wd, momentum, gscale, coef=None):
    """k_rmsprop, as adam_intervals: s = fmaf(alpha, sq, fl(fl(fl(1-alpha) gi) gi)); avg = fl(sqrtf(s) + eps);
    momentum > 0: b = fmaf(momentum, buf, fl(gi / avg)), p = fl(pi - fl(lr b)); else p = fl(pi - fl(lr fl(gi / avg)))"""
    lr, alpha, eps, momentum = f32(lr), f32(alpha), f32(eps), f32(momentum)
    s = lambda c: _iv(c, g)
    gi = _opt_grad(p, g, wd, gscale, coef)
    si = ifma(s(alpha), _iv(sq), imul(imul(s(_om(alpha)), gi, 1), gi, 1))
    si = Interval(si.lo.clamp_min(0.0), si.hi)
    avg = iadd(isqrt(si), s(eps), 1)
    r = idiv(gi, avg, 1)
    out = dict(sq=si)
    if momentum > 0:
        r = ifma(s(momentum), _iv(buf), r)
        out["buf"] = r
    out["p"] = iadd(_iv(p), imul(s(lr), r, 1), 1, -1.0)
    return out


def sgd_intervals(p, g, buf, lr, momentum, dampening, wd, nesterov, step, gscale, coef=None):
    """k_sgd: momentum != 0: b = gi on the first step, else fmaf(momentum, buf, fl(fl(1-dampening) gi)); nesterov:
    gi = fmaf(momentum, b, gi), else b; p = fl(pi - fl(lr gi))"""
    lr, momentum, dampening = f32(lr), f32(momentum), f32(dampening)
    s = lambda c: _iv(c, g)
    gi = _opt_grad(p, g, wd, gscale, coef)
    out = {}
    if momentum != 0.0:
        b = gi if step == 1 else ifma(s(momentum), _iv(buf), imul(s(_om(dampening)), gi, 1))
        out["buf"] = b
        gi = ifma(s(momentum), b, gi) if nesterov else b
    out["p"] = iadd(_iv(p), imul(s(lr), gi, 1), 1, -1.0)
    return out


def opt_coef_interval(partial, max_norm, like):
    """(norm, coef, Interval of coef) from the fp64 partial table handed to a *_step_ex launch, by tests/gradclip_ref.py: the
    tests' tables hold a few values whose sum is exact in any order, so norm is the one fp32 rounding of the fp64 root; the
    clip's fp32 division is taken at one ulp (it is IEEE in this build; the stats block's last_coef is compared separately)"""
    import numpy as np
    import gradclip_ref as R
    norm = np.float32(np.sqrt(np.float64(sum(partial))))
    c = R.coef(norm, max_norm)
    cv = float(c)
    if cv != cv:
        return norm, c, None
    iv = _iv(cv, like) if cv == 1.0 else Interval(*(torch.tensor(v, dtype=torch.float64, device=like.device)
                                                    for v in (cv * (1 - 2 * U32), cv * (1 + 2 * U32))))
    return norm, c, iv


def check_ema(ema_dev, d, ema_prev, p_dev, what, family="optimizers"):
    """the EMA behind p: gradclip_ref.ema_bound around the p the device stored"""
    import gradclip_ref as R
    want, bound = R.ema_bound(d, ema_prev.cpu().numpy(), p_dev.cpu().numpy())
    return _assert_bound(ema_dev.cpu(), torch.from_numpy(want), torch.from_numpy(bound) + TINY32, what, family)


_OPT_BUFS = {"adam": ("p", "g", "m", "v"), "rmsprop": ("p", "g", "v", "buf"), "sgd": ("p", "g", "buf")}


def opt_case(kind, st, a, offset, ex=None, family="optimizers"):
    """ONE launch of mnas_<kind>_step (ex None) or mnas_<kind>_step_ex from the state st (cpu fp32 tensors p, g, m, v, buf, ema),
    every buffer a guarded view at element `offset`; a: the keyword arguments of <kind>_intervals.  ex: dict(partial=[fp64 values
    whose sum is exact], max_norm, skip, ema (bool), decay).  Every output inside its bracket, g (and an unused momentum buffer)
    bitwise untouched, canaries on both sides intact; _ex: the EMA inside gradclip_ref.ema_bound around the p the device stored,
    the stats block as documented, a skipped step leaves every buffer bitwise untouched.  -> worst error / bracket."""
    import numpy as np
    lib = L.load()
    names = _OPT_BUFS[kind] + (("ema",) if ex is not None and ex["ema"] else ())
    n = st["p"].numel()
    buf, chk = {}, {}
    for k in names:
        buf[k], chk[k] = guarded((n,), torch.float32, offset=offset)
        buf[k].copy_(st[k])
    before = {k: v.clone() for k, v in buf.items()}
    P = lambda k: buf[k].data_ptr()
    tail, sfx = [], ""
    if ex is not None:
        partial = torch.tensor(ex["partial"], dtype=torch.float64, device="cuda")
        stats = torch.zeros(4, dtype=torch.int64, device="cuda")
        e = L.MnasOptExtra(partial=partial.data_ptr(), nparts=len(ex["partial"]), max_norm=ex["max_norm"], skip_nonfinite=ex["skip"],
                           ema=P("ema") if ex["ema"] else None, ema_decay=ex["decay"], stats=stats.data_ptr(), update_stats=1)
        tail, sfx = [C.byref(e)], "_ex"
    fn = getattr(lib, "mnas_%s_step%s" % (kind, sfx))
    if kind == "adam":
        rc = fn(P("p"), P("g"), P("m"), P("v"), n, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["step"], a["gscale"], *tail, L.cur_stream())
    elif kind == "rmsprop":
        rc = fn(P("p"), P("g"), P("v"), P("buf"), n, a["lr"], a["alpha"], a["eps"], a["wd"], a["momentum"], a["gscale"], *tail, L.cur_stream())
    else:
        rc = fn(P("p"), P("g"), P("buf"), n, a["lr"], a["momentum"], a["dampening"], a["wd"], a["nesterov"], a["step"], a["gscale"],
                *tail, L.cur_stream())
    L.check(rc, kind)
    what = "%s%s n %d offset %d %r" % (kind, sfx, n, offset, a)
    for k in names:
        chk[k](what + " " + k)
    bits_equal(buf["g"], before["g"], what + " g")
    coef = None
    if ex is not None:
        norm, c, coef = opt_coef_interval(ex["partial"], ex["max_norm"], before["p"])
        raw = L.MnasGradStats()
        host = stats.cpu()
        C.memmove(C.byref(raw), host.data_ptr(), 32)
        skipped = bool(ex["skip"]) and not np.isfinite(norm)
        assert raw.steps == 1 and raw.skipped_steps == int(skipped), what
        if np.isfinite(norm):
            assert abs(raw.last_norm - float(norm)) <= 2.0 ** -23 * float(norm), what
            assert abs(raw.last_coef - float(c)) <= 2.0 ** -22 * float(c) and (raw.last_coef == 1.0) == (float(c) == 1.0), what
            assert raw.clipped_steps == int(float(c) < 1.0), what
        else:
            assert not np.isfinite(raw.last_norm), what
        if skipped:
            for k in names:
                bits_equal(buf[k], before[k], what + " skipped step, " + k)
            return 0.0
    b = before
    if kind == "adam":
        ivs = adam_intervals(b["p"], b["g"], b["m"], b["v"], coef=coef, **a)
    elif kind == "rmsprop":
        ivs = rmsprop_intervals(b["p"], b["g"], b["v"], b["buf"], coef=coef, **a)
        ivs["v"] = ivs.pop("sq")
    else:
        ivs = sgd_intervals(b["p"], b["g"], b["buf"], coef=coef, **a)
    worst = 0.0
    for k in _OPT_BUFS[kind]:
        if k in ivs:
            worst = max(worst, check_interval(buf[k], ivs[k], what + " " + k, family))
        else:
            bits_equal(buf[k], before[k], what + " " + k + " (not an output)")
    if ex is not None and ex["ema"]:
        worst = max(worst, check_ema(buf["ema"], ex["decay"], before["ema"], buf["p"], what + " ema", family))
    return worst


# ---- the multi-label loss (csrc/mnas_mlabel.hip: k_mlabel_row, k_mlabel_batch, k_mlabel_scale) and HardDice ----------------------------
# Same conventions.  mnas_mlabel.o is built with -ffp-contract=on: a multiply may fuse with the add of the SAME expression, so
# `- z*t +` and `ls += e*w` are bracketed as the hull of their fused and unfused forms.  expf, log1pf, logf and the divisions are
# taken at ONE ULP (2u relative; a subnormal result: 2^-149 absolute), the assumption ce_intervals makes.
E64 = 2.0 ** -52          # one double ulp, relative


def _f32r(x):
    """round a double tensor to fp32 (to nearest even) and back: monotone, so it maps a bracket's ends to the rounded bracket's"""
    return x.float().double()


def _ulp1(lo, hi):
    """a one-ulp fp32 function of a value known to lie between the fp64 results lo <= hi (the host's own error: D64)"""
    f = 2 * U32 + D64
    return lo - f * lo.abs() - TINY32, hi + f * hi.abs() + TINY32


def _dw(lo, hi, n=1):
    """n double roundings (or n one-ulp double functions) of a value in [lo, hi]"""
    return lo - n * E64 * lo.abs(), hi + n * E64 * hi.abs()


def _dmul(a, b, n=1):
    p = imul(a, b, 0)
    return Interval(*_dw(p.lo, p.hi, n))


ML_SHAPES = [(1, 1), (3, 5), (5, 257), (2, 1000), (3, 1024), (3, 1028), (2, 2052), (3, 1027), (257, 3), (513, 4)]
ML_KINDS = ["scale0.5", "scale8", "scale30", "edges", "confident", "soft", "pow2w", "sparse"]
ML_EDGE_Z = [0.0, -0.0, 17.0, -17.0, 18.0, -18.0, 88.0, -88.0, 90.0, -90.0, 104.0, -104.0, 200.0, -200.0]
ML_LIVE_COLS = (0, 255, 256, 1023, 1024)
ML_FOCAL = ((1.0, 0.25), (2.0, 0.25), (3.5, 0.75))          # (focus_param, balance_param) of the focal cases
ML_BIG = (1100, 1000)                                       # N*C > 4096*256: k_mlabel_scale's grid-stride second trip


def mlabel_live(N, C_):
    """the sparse probe's live element of every row: columns 0, 255, 256, 1023, 1024 and C-1 (those that exist) in turn"""
    cols = sorted({c for c in ML_LIVE_COLS + (C_ - 1,) if c < C_})
    return [(n, cols[n % len(cols)]) for n in range(N)]


def mlabel_inputs(kind, N, C_):
    """(z, t, w) fp32 [N][C] of the multi-label bound tests (CPU proofs and GPU cases read the same).  scale*: logits leaning
    towards the labels times 0.5 / 8 / 30; edges: z through +-0 and |z| = 17, 18 (ea below 2^-24), 88, 90 (ea subnormal), 104, 200
    (ea zero), against both targets; confident: z = +-(18..30) agreeing with t everywhere (log1pf(ea) is the whole loss); soft:
    targets 0, 0.3, 0.7, 1; pow2w: weights 2^-12..2^12 and exact zeros; sparse: ONE live weight per row (mlabel_live)."""
    g = torch.Generator().manual_seed(N * 1000 + C_ + 7)
    t = (torch.rand(N, C_, generator=g) < 0.4).float()
    u = torch.randn(N, C_, generator=g)
    w = 0.25 + 1.5 * torch.rand(N, C_, generator=g)
    if kind.startswith("scale"):
        return (u + 0.5 * (2 * t - 1)) * float(kind[5:]), t, w
    if kind == "edges":
        i = torch.arange(N * C_)
        z = torch.tensor(ML_EDGE_Z)[i % len(ML_EDGE_Z)].view(N, C_)
        return z, ((i // len(ML_EDGE_Z)) % 2).float().view(N, C_), w
    if kind == "confident":
        return (2 * t - 1) * (18.0 + 12.0 * torch.rand(N, C_, generator=g)), t, w
    z = (u + 0.5 * (2 * t - 1)) * 2.0
    if kind == "soft":
        return z, torch.tensor([0.0, 0.3, 1.0, 0.7])[torch.randint(0, 4, (N, C_), generator=g)], w
    if kind == "pow2w":
        w = torch.pow(torch.tensor(2.0), torch.randint(-12, 13, (N, C_), generator=g).float())
        w[torch.rand(N, C_, generator=g) < 0.2] = 0.0
        return z, t, w
    assert kind == "sparse"
    w = torch.zeros(N, C_)
    for (n, c) in mlabel_live(N, C_):
        w[n, c] = 1.0
    return z, t, w


def mlabel_inv(N, C_):
    """r.inv of mnas_mlabel_bce, bit for bit: (float)(1.0 / ((double)N * (double)C))"""
    return float(torch.tensor(1.0 / (float(N) * float(C_)), dtype=torch.float64).float())


def mlabel_trips(C_, vec):
    """terms a lane of k_mlabel_row adds: ceil(C/256) on the scalar path, 4 ceil(C/1024) on the vector path"""
    return 4 * -(-C_ // 1024) if vec else -(-C_ // 256)


def mlabel_batch_intervals(rows_dev, N, C_, focal, gamma, balance):
    """k_mlabel_batch's loss (and, focal, the gradient's factor s) from the loss_rows the device stored (exact data): the double
    sum in a fixed order (relative D64 = 2^-48 of sum|rows|, all of it the device's: the host's centre is math.fsum's correctly
    rounded sum), one double division by N*C, ONE rounding to fp32: b.  Focal, all in
    double, operation by operation at one double ulp each (two where the host's own exp / pow is in the chain): pt = exp(-b),
    om = 1 - pt, loss = (float)((balance * pow(om, g)) * b), s = (float)((balance * pow(om, g - 1)) * (om + (g * pt) * b)).  om
    cancels for a tiny b: it is then known to 2^-52 / b relative only, and so are the loss and s -- the kernel's own operation.
    gamma, balance: the fp32 values the ABI passes.  -> dict(b=, loss=, s= (None without focal)) of 0-dim Intervals."""
    r = rows_dev.detach().cpu().double().reshape(-1)                 # (N numbers: on the host, whichever device the rest runs on)
    import math
    S = torch.tensor(math.fsum(r.tolist()), dtype=torch.float64)    # (the bracket's centre: the correctly rounded sum, so that D64
    Sa = torch.tensor(math.fsum(r.abs().tolist()), dtype=torch.float64)   # is the device's allowance alone)
    den = float(N) * float(C_)
    lo, hi = (S - D64 * Sa) / den, (S + D64 * Sa) / den
    lo, hi = _dw(lo, hi, 1)
    b = Interval(_f32r(lo), _f32r(hi))
    if not focal:
        return dict(b=b, loss=b, s=None)
    g, bal = _iv(f32(gamma), r), _iv(f32(balance), r)
    pt = Interval(*_dw(torch.exp(-b.hi), torch.exp(-b.lo), 2))
    olo, ohi = _dw(1.0 - pt.hi, 1.0 - pt.lo, 1)
    om = Interval(olo.clamp_min(0.0), ohi.clamp_min(0.0))
    pw = Interval(*_dw(torch.pow(om.lo, g.lo), torch.pow(om.hi, g.lo), 2))
    pw1 = Interval(*_dw(torch.pow(om.lo, g.lo - 1.0), torch.pow(om.hi, g.lo - 1.0), 2))
    loss = _dmul(_dmul(bal, pw), b)
    gp = _dmul(_dmul(g, pt), b)
    inner = Interval(*_dw(om.lo + gp.lo, om.hi + gp.hi, 1))
    s = _dmul(_dmul(bal, pw1), inner)
    return dict(b=b, loss=Interval(_f32r(loss.lo), _f32r(loss.hi)), s=Interval(_f32r(s.lo), _f32r(s.hi)))


def mlabel_intervals(z, t, w, N, C_, focal, gamma, balance, vec, rows_dev=None):
    """Brackets of every output of mnas_mlabel_bce, by interval propagation through ml_elem as written; z, t, w (None: no weights)
    fp32 [N][C] as the device reads them, on any device (the fp64 work runs where z lives).
      ea = expf(-|z|) and log1pf(ea) at one ulp; m = fmaxf(z, 0) exact; A = m - z*t: fl(m - z t) fused, fl(m - fl(z t)) unfused,
      the hull; e = fl(A + log1pf(ea)); the row's term e*w: exact inside a fused ls += e*w, fl(e w) unfused, the hull (w NULL: e).
      sg: z >= 0 (-0.0 too): 1/fl(1 + ea); z < 0: ea/fl(1 + ea) -- each branch bracketed on its own elements, division one ulp;
      dlogits = fl(fl(w fl(sg - t)) inv), inv = mlabel_inv(N, C) (no multiply feeds an add there: nothing to fuse).  sg - t
      cancels for a confident true class; that is the kernel's arithmetic and the bracket follows it.
      row sums: a lane adds T = mlabel_trips(C, vec) terms, then 6 butterfly adds and 3 adds of the four waves:
          |row - sum mid(e w)| <= (T + 9) 2^-23 sum|e w| + sum half(e w)        (check_sum_bound's form; no term excluded).
    rows_dev (the device's loss_rows, scratch byte 8 N): adds mlabel_batch_intervals' b, loss and s; focal: dlogits is the unscaled
    bracket times the bracket of s, one rounding more (k_mlabel_scale).
    -> dict(dl, dl_unscaled, ew, rows, row_half, [b, loss, s])."""
    z, t = z.double(), t.double()
    one = _iv(1.0, z)
    a = z.abs()
    elo, ehi = _ulp1(torch.exp(-a), torch.exp(-a))
    ea = Interval(elo.clamp_min(0.0), ehi)
    llo, lhi = _ulp1(torch.log1p(ea.lo), torch.log1p(ea.hi))
    l1 = Interval(llo.clamp_min(0.0), lhi)
    m, zt = z.clamp_min(0.0), z * t                                   # (fp32 x fp32: exact in double)
    fl_, fh = _w32(m - zt, m - zt, 1)
    zr = _f32r(zt)                                                    # (the unfused product: ONE known fp32 number)
    ul, uh = _w32(m - zr, m - zr, 1)
    A = Interval(torch.minimum(fl_, ul), torch.maximum(fh, uh))
    e = iadd(A, l1, 1)
    if w is None:
        ew, wv = e, None
    else:
        wv = _iv(w.double())
        ex, un = imul(e, wv, 0), imul(e, wv, 1)
        ew = Interval(torch.minimum(ex.lo, un.lo - TINY32), torch.maximum(ex.hi, un.hi + TINY32))
    T = mlabel_trips(C_, vec)
    row_half = (T + 9) * 2.0 ** -23 * ew.amax.sum(1) + ew.half.sum(1)
    rows = Interval(ew.mid.sum(1) - row_half, ew.mid.sum(1) + row_half)
    d = iadd(one, ea, 1)
    sp, sn = idiv(one, d, 1, 2), idiv(ea, d, 1, 2)
    pos = z >= 0
    sg = Interval(torch.where(pos, sp.lo, sn.lo), torch.where(pos, sp.hi, sn.hi))
    df = iadd(sg, _iv(t), 1, -1.0)
    if wv is not None:
        df = imul(wv, df, 1)
    dl0 = imul(df, _iv(mlabel_inv(N, C_), z), 1)
    dl0 = Interval(dl0.lo - TINY32, dl0.hi + TINY32)
    out = dict(dl=dl0, dl_unscaled=dl0, ew=ew, rows=rows, row_half=row_half)
    if rows_dev is not None:
        out.update(mlabel_batch_intervals(rows_dev, N, C_, focal, gamma, balance))
        if focal:
            s = out["s"]
            sc = imul(dl0, Interval(s.lo.to(z.device), s.hi.to(z.device)), 1)
            out["dl"] = Interval(sc.lo - TINY32, sc.hi + TINY32)
    elif focal:
        out["dl"] = None
    return out


def mlabel_probe_visible(iv, live, what):
    """the sparse probe of the multi-label rows: every live element's loss term (lower end) exceeds twice its row's bound"""
    lo = iv["ew"].lo
    for (n, c) in live:
        assert float(lo[n, c]) > 2 * float(iv["row_half"][n]), "%s: the live term (%d, %d) would not be seen" % (what, n, c)


def dice_interval(I, P, T, deduct):
    """ml_dice: 0 when I <= 0; else U = P + T - (deduct ? I : 0), a = (float)(2 I), b = (float)U each rounded as the int64 ->
    fp32 conversion rounds (to nearest even; exact below 2^24), q = a / b and logf(q) at one ulp, v = fl(1 + logf(q)), the clamp
    to [0, 1] applied to both ends.  -> 0-dim Interval."""
    if I <= 0:
        return _iv(0.0)
    U = P + T - (I if deduct else 0)
    a, b = _f32r(torch.tensor(float(2 * I), dtype=torch.float64)), _f32r(torch.tensor(float(U), dtype=torch.float64))
    q = idiv(Interval(a, a), Interval(b, b), 1, 2)
    lg = Interval(*_ulp1(torch.log(q.lo), torch.log(q.hi)))
    v = iadd(_iv(1.0), lg, 1)
    return Interval(v.lo.clamp(0.0, 1.0), v.hi.clamp(0.0, 1.0))
